"""Feldman share checks recorded FROM THE REFERENCE'S OWN DKG CLIENT (run in the build container only).

Imports agent/dkg/SA_ClientAgent.py read-only from /root/reference under tests/golden/refshim.py (as
make_ref_golden.py imports the Flamingo agents) and drives its own sendShareCommitments (:180-212)
and verify_commitment (:219-228).  Only data is recorded: each dealer's commitments and shares, and
the reference's verdict on every (dealer, receiver) row and on three tampered twins of it:

  share+1    the share plus one;
  wrong_id   the right share checked under another receiver's id (x);
  swap       one commitment replaced by another dealer's commitment of the same term.

n = 6 (threshold int(n/3) + 1 = 3: 4 commitments): the full 6 x 6 grid.
n = 60 (22 commitments): dealers 1-3 against receivers 1, 2, 59 and 60.

``python tests/golden/make_dkg_golden.py`` rewrites dkg_golden.json; tests/test_dkg_cpu.py replays
generate() against it where the reference is present.  A point is 64 bytes x || y in hex, infinity
(pycryptodome's EccPoint(0, 0)) 64 zero bytes; a share 32 bytes, big endian.
"""
from __future__ import annotations

import contextlib
import io
import json
import os
import random
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "dkg_golden.json")
REF = "/root/reference"
GROUPS = ((6, range(1, 7), range(1, 7)), (60, (1, 2, 3), (1, 2, 59, 60)))

_CA = None


def _client_module():
    """The reference's dkg client module, imported once under the shim."""
    global _CA
    if _CA is None:
        sys.path.insert(0, HERE)
        import refshim
        refshim.install()
        sys.path.insert(0, REF)
        from util import util
        util.silent_mode = True
        import agent.dkg.SA_ClientAgent as CA
        _CA = (CA, refshim)
    return _CA


class _Outbox:
    """The kernel calls sendShareCommitments makes: the message is kept, nothing is delivered."""

    def __init__(self):
        self.sent = []

    def sendMessage(self, sender, recipient, msg, delay=0, tag="communication"):
        self.sent.append(msg)

    def setAgentComputeDelay(self, sender, requestedDelay):
        pass


def _pt_hex(pt) -> str:
    return (int(pt.x).to_bytes(32, "big") + int(pt.y).to_bytes(32, "big")).hex()


def _group(n: int, dealers, receivers) -> dict:
    import numpy as np
    CA, refshim = _client_module()
    refshim.DRBG.reset(f"dkg-golden-{n}".encode())   # random_polynomial's coefficients (secure_randint)
    random.seed(f"dkg-golden-{n}")                   # my_random_si (random.randint, :188)
    ids = sorted(set(dealers) | set(receivers))
    agents, box = {}, _Outbox()
    for i in ids:
        a = CA.SA_ClientAgent(id=i, name=f"DKG Client Agent {i}", type="ClientAgent", num_clients=n,
                              random_state=np.random.RandomState(i))
        a.kernel = box
        agents[i] = a
    dealt = {}
    for d in dealers:
        del box.sent[:]
        agents[d].sendShareCommitments()
        (msg,) = box.sent
        assert msg.body["msg"] == "share_and_commit" and msg.body["sender"] == d
        dealt[d] = (msg.body["si_shares"], msg.body["commitments"])
    T = agents[ids[0]].threshold + 1
    dl, rc = list(dealers), list(receivers)
    records = []
    for d in dl:
        shares, com = dealt[d]
        other = dl[(dl.index(d) + 1) % len(dl)]
        for r in rc:
            x, y = shares[r]
            assert x == r
            r2 = rc[(rc.index(r) + 1) % len(rc)]
            k = (d + r) % T
            swapped = list(com)
            swapped[k] = dealt[other][1][k]
            for kind, who, sh, cs, swap in (("honest", r, y, com, None), ("share+1", r, y + 1, com, None),
                                            ("wrong_id", r2, y, com, None), ("swap", r, y, swapped, [k, other])):
                with contextlib.redirect_stdout(io.StringIO()):
                    ok = agents[who].verify_commitment((who, sh), cs)
                records.append({"kind": kind, "dealer": d, "x": who, "share": int(sh).to_bytes(32, "big").hex(),
                                "swap": swap, "ok": bool(ok)})
    return {"n": n, "T": T,
            "commitments": {str(d): [_pt_hex(c) for c in dealt[d][1]] for d in dl},
            "records": records}


def generate() -> dict:
    return {"generator": "tests/golden/make_dkg_golden.py: agent/dkg/SA_ClientAgent.py (sendShareCommitments, "
                         "verify_commitment) of /root/reference under tests/golden/refshim.py",
            "groups": [_group(n, d, r) for n, d, r in GROUPS]}


def load() -> dict:
    with open(OUT) as f:
        return json.load(f)


def rows(fixture: dict):
    """Every record as (group n, T, commitments [T] of 64 bytes, x, share bytes, expected verdict, label)."""
    for g in fixture["groups"]:
        for rec in g["records"]:
            com = [bytes.fromhex(h) for h in g["commitments"][str(rec["dealer"])]]
            if rec["swap"]:
                k, other = rec["swap"]
                com[k] = bytes.fromhex(g["commitments"][str(other)][k])
            yield (g["n"], g["T"], com, rec["x"], bytes.fromhex(rec["share"]), rec["ok"],
                   f'n{g["n"]}-d{rec["dealer"]}-x{rec["x"]}-{rec["kind"]}')


if __name__ == "__main__":
    g = generate()
    with open(OUT, "w") as f:               # one record per line
        f.write('{"generator": %s,\n"groups": [\n' % json.dumps(g["generator"]))
        for gi, grp in enumerate(g["groups"]):
            f.write('{"n": %d, "T": %d,\n"commitments": %s,\n"records": [\n%s]}%s\n' % (
                grp["n"], grp["T"], json.dumps(grp["commitments"], sort_keys=True),
                ",\n".join(json.dumps(r, sort_keys=True) for r in grp["records"]),
                "," if gi + 1 < len(g["groups"]) else ""))
        f.write("]}\n")
    print(OUT, os.path.getsize(OUT), "bytes")
