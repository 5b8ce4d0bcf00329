"""Helpers of the DKG agent tests (tests/test_dkg_cpu.py, tests/test_dkg_gpu.py).  No test functions.

Cheating is injected by subclasses of the client agent that override the method building the
`share_and_commit` body (SA_ClientAgent.shareCommitBody); the product code has no hook for it.
"""
from __future__ import annotations

from flamingo_amd import crypto as C
from flamingo_amd.abides import config_dkg
from flamingo_amd.abides.dkg import SA_ClientAgent, keygen

N = C.N
VICTIM = 3


class BadShareThenGood(SA_ClientAgent):
    """Sends member VICTIM a wrong share, and answers its complaint with the right one."""

    def shareCommitBody(self):
        body = dict(super().shareCommitBody())
        x, y = body["si_shares"][VICTIM]
        body["si_shares"] = dict(body["si_shares"])
        body["si_shares"][VICTIM] = (x, (y + 1) % N)
        return body


class BadShareTwice(BadShareThenGood):
    """Sends member VICTIM a wrong share, and broadcasts the same wrong share after the complaint."""

    def shareCommitBody(self):
        body = super().shareCommitBody()
        self.si_shares_with_recvrs = dict(self.si_shares_with_recvrs)
        self.si_shares_with_recvrs[VICTIM] = body["si_shares"][VICTIM]
        return body


def run(n: int, seed: int, gpu: bool, cheats=None) -> dict:
    """One key generation with a deterministic latency (no message is late); cheats: {id: class}."""
    keygen.configure(gpu_dkg=gpu)
    try:
        return config_dkg.simulate(n, seed, latency="deterministic", client_classes=cheats)
    finally:
        keygen.configure(gpu_dkg=True)


def messages(res) -> list:
    """Everything the server forwarded, in order, as comparable values."""
    return [(to, repr(sorted(body.items(), key=lambda kv: kv[0]))) for to, body in res["server"].sent]


def check_keys(res, qual_expected) -> None:
    """Every member agrees on QUAL and on the group key; the group key is the sum of the QUAL dealers'
    C_0; any degree + 1 key shares interpolate to one secret whose public point is the group key; and
    each share is the sum of what the QUAL dealers dealt that member."""
    members = res["members"]
    n = len(res["agents"]) - 1
    assert sorted(members) == list(range(1, n + 1))
    qual, key = config_dkg.agreed(members)
    assert qual == sorted(qual_expected)
    agents = {a.id: a for a in res["agents"][1:]}
    want = None
    for d in qual:
        want = C.add(want, agents[d].my_commitments[0])
    assert key == want and key is not None
    t = agents[1].poly_degree + 1
    ids = sorted(members)
    sk = config_dkg.interpolated_key(members, ids[:t])
    assert C.mul(sk) == key
    assert config_dkg.interpolated_key(members, ids[-t:]) == sk
    assert config_dkg.interpolated_key(members, ids[1:t + 1]) == sk
    for j in ids:       # a QUAL dealer's own record is what it truly dealt (a cheat that stays in QUAL keeps it right)
        dealt = sum(agents[d].si_shares_with_recvrs[j][1] for d in qual) % N
        assert members[j]["sk_share"] == (j, dealt)
