"""The DKG agents without a GPU.  The agents' engine is replaced by a double that brings none of the
batched calls, which leaves dealing and checking on the host path (seeds.shamir_share, crypto.mul,
crypto.feldman_verify) -- the route tests/test_abides_protocol_cpu.py takes for the Flamingo agents:

* an honest run: QUAL is everyone and the keys are consistent;
* a dealer that sends one member a bad share and then broadcasts a good one stays in QUAL; one that
  broadcasts the bad one is excluded, and the keys stay consistent over the smaller QUAL;
* the message surface and the wake-up schedule are the reference's;
* the batched path's draw of a dealer's coefficients is the host path's stream, value for value;
* Flamingo with dkg=True on the CPU oracle engine: the final sum is right with dropouts, no
  COMMITTEE_SHARED_SK is sent, and the system's private key cannot be read.
The GPU versions of the same runs are in tests/test_dkg_gpu.py."""
import copy

import numpy as np
import pytest

import dkg_cases as D
from flamingo_amd import crypto as C


class NoBatchEngine:
    """An engine without the dealing and checking calls: keygen.on_gpu() is False with it."""


@pytest.fixture
def host_engine(monkeypatch):
    from flamingo_amd.abides.flamingo import protocol
    monkeypatch.setattr(protocol, "_engine", NoBatchEngine())
    yield
    protocol.configure(committee=60, dkg=False)


def test_honest_run(host_engine):
    from flamingo_amd.abides.dkg import keygen
    res = D.run(6, 7, gpu=True)          # the double has no batched calls: the host path all the same
    assert not keygen.on_gpu()
    D.check_keys(res, range(1, 7))
    assert res["agents"][1].poly_degree == 3 and len(res["agents"][1].my_commitments) == 4


def test_message_surface_and_schedule(host_engine):
    import pandas as pd
    res = D.run(6, 7, gpu=False)
    sent = res["server"].sent
    kinds = [b["msg"] for _, b in sent]
    assert kinds == ["SHARE_AND_COMMIT"] * 6 + ["ACCEPT_OR_COMPLAIN"] * 6 + ["FORWARD_SHARE"] * 6 + ["BCAST_QUAL"] * 6
    assert [to for to, _ in sent] == [1, 2, 3, 4, 5, 6] * 4
    first = sent[0][1]
    assert set(first) == {"msg", "shares", "commitments"}
    assert sorted(first["shares"]) == [1, 2, 3, 4, 5, 6] and first["shares"][4][0] == 1      # (x, y) at member 1's point
    assert set(sent[6][1]) == {"msg", "complaints_from"} and sent[6][1]["complaints_from"] == []
    assert set(sent[12][1]) == {"msg", "bcast_shares"}
    assert set(sent[18][1]) == {"msg", "output"} and sorted(sent[18][1]["output"]) == [1, 2, 3, 4, 5, 6]
    # the server's wake-ups: start, +1 s, +3 s, +2 s, +2 s (SA_ServiceAgent.py:166-261)
    wakes = res["server"].wake_times
    assert wakes[0] == pd.to_datetime("2023-01-01")
    assert [b - a for a, b in zip(wakes, wakes[1:])] == [pd.Timedelta(t) for t in ("1s", "3s", "2s", "2s")]


def test_complaint_answered_by_a_good_share_keeps_the_dealer(host_engine):
    res = D.run(6, 7, gpu=False, cheats={2: D.BadShareThenGood})
    sent = res["server"].sent
    complaints = {to: b["complaints_from"] for to, b in sent if b["msg"] == "ACCEPT_OR_COMPLAIN"}
    assert complaints[2] == [D.VICTIM] and all(v == [] for d, v in complaints.items() if d != 2)
    bcast = [b for _, b in sent if b["msg"] == "FORWARD_SHARE"][0]["bcast_shares"]
    assert list(bcast[2]) == [D.VICTIM] and all(not v for d, v in bcast.items() if d != 2)
    D.check_keys(res, range(1, 7))


def test_bad_broadcast_share_excludes_the_dealer(host_engine):
    res = D.run(6, 7, gpu=False, cheats={2: D.BadShareTwice})
    D.check_keys(res, [1, 3, 4, 5, 6])


def test_command_line_driver(host_engine, capsys):
    """python -m flamingo_amd.abides -c dkg: the cubic latency model of the reference's config, the
    closing agreement check and its printed summary"""
    from flamingo_amd.abides.config_dkg import run
    res = run(["-c", "dkg", "-n", "6", "-s", "7", "-k", "--host_dkg"])
    assert res["qual"] == [1, 2, 3, 4, 5, 6] and res["group_key"] is not None
    out = capsys.readouterr().out
    assert "all agree on QUAL (6 dealers) and on one group key: True" in out
    assert "4 key shares interpolate to the group key's secret: True" in out and "path: host" in out


def test_batched_draw_is_the_host_paths_stream(host_engine):
    from flamingo_amd.abides.dkg import SA_ClientAgent, keygen
    keygen.configure()
    a = SA_ClientAgent(id=1, name="a", type="ClientAgent", num_clients=6, random_state=np.random.RandomState(11))
    b = copy.deepcopy(a)
    coeffs = keygen._draw(a)
    shares, commitments = keygen._deal_host(b)
    assert len(coeffs) == 4 and commitments == [C.mul(c) for c in coeffs]
    assert shares == {j: (j, sum(c * j ** k for k, c in enumerate(coeffs)) % C.N) for j in range(1, 7)}
    assert a.random_state.randint(0, 1 << 30) == b.random_state.randint(0, 1 << 30)       # the streams stay in step
    keygen.configure()


def test_flamingo_with_dkg_on_the_oracle_engine(monkeypatch):
    from test_abides_protocol_cpu import OracleEngine
    from flamingo_amd.abides.config_flamingo import run
    from flamingo_amd.abides.flamingo import protocol
    from flamingo_amd.abides.kernel import Kernel
    monkeypatch.setattr(protocol, "_engine", OracleEngine())
    seen = []
    send = Kernel.sendMessage

    def spy(self, sender=None, recipient=None, msg=None, delay=0, tag=None):
        seen.append(msg.body.get("msg"))
        return send(self, sender, recipient, msg, delay=delay, tag=tag)
    monkeypatch.setattr(Kernel, "sendMessage", spy)
    try:
        res = run(["-c", "flamingo", "-n", "32", "-i", "2", "-s", "5", "-k", "--vector_len", "1000",
                   "--committee_size", "6", "--root_seed_hex", "11" * 32, "--round_time", "30",
                   "--offline", "3,9,20", "--dkg"])
        srv = res["server"]
        assert sorted(srv.results) == [1, 2]
        for it, out in srv.results.items():
            assert np.all(out == srv.online_counts[it]), it
        assert len(srv.recon_symbol) > 0
        assert "COMMITTEE_SHARED_SK" not in seen and "share_and_commit" in seen and "VECTOR" in seen
        keys = protocol.pki(32)
        with pytest.raises(RuntimeError, match="nobody holds"):
            keys.system_sk
        assert keys.system_pk == protocol._dkg_result[0]
    finally:
        protocol.configure(committee=60, dkg=False)
    # the switch off again: the default set-up as before
    monkeypatch.setattr(protocol, "_engine", OracleEngine())
    assert protocol.pki(32).system_sk > 0 and not protocol.dkg_on()
    protocol.configure(committee=60)
