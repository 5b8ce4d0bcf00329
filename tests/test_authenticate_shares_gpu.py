"""protocol.configure(authenticate_shares=True) on the real engine: the scenarios of
tests/test_authenticate_shares_cpu.py (its simulate and tamper functions) with the clients' shares
sealed in one flm_aes_gcm_seal launch per iteration and each member's opened in one
flm_aes_gcm_open launch, and the batched path against the per-share host path, byte for byte."""
from __future__ import annotations

import pytest

from test_authenticate_shares_cpu import (COMMITTEE, KNOWN_CLIENT_MESSAGES, N, committee, dropouts, flip_bit,
                                          refused_exactly, replay, simulate, sums_hold)

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _switches_back():
    from flamingo_amd.abides.flamingo import protocol
    yield
    protocol.configure(committee=60, authenticate_shares=False, gpu_deal=True)


@pytest.fixture
def launches(monkeypatch):
    """counts the engine's seal and open calls: {"seal": [rows per call], "open": [...]}"""
    from flamingo_amd.engine import MaskEngine
    seen = {"seal": [], "open": []}
    seal, open_ = MaskEngine.aes_gcm_seal_wire, MaskEngine.aes_gcm_open_wire
    monkeypatch.setattr(MaskEngine, "aes_gcm_seal_wire",
                        lambda self, keys, *a, **kw: seen["seal"].append(len(keys)) or seal(self, keys, *a, **kw))
    monkeypatch.setattr(MaskEngine, "aes_gcm_open_wire",
                        lambda self, keys, *a, **kw: seen["open"].append(len(keys)) or open_(self, keys, *a, **kw))
    return seen


def test_option_off_sends_what_it_always_sent(monkeypatch, launches):
    members = committee()
    off = dropouts(members)
    run = simulate(monkeypatch, False, offline=off)
    assert run.fields == {32} and run.kinds == KNOWN_CLIENT_MESSAGES and run.refused == []
    assert launches == {"seal": [], "open": []}
    sums_hold(run, off)


def test_option_on_batched_and_host_paths_send_the_same_bytes(monkeypatch, launches):
    members = committee()
    off = dropouts(members)
    host = simulate(monkeypatch, True, gpu_deal=False, offline=off)
    assert launches == {"seal": [], "open": []}, "gpu_deal=False must seal and open on the host"
    gpu = simulate(monkeypatch, True, gpu_deal=True, offline=off)
    # one seal launch per iteration over every online client's shares; one open launch per member and iteration
    assert launches["seal"] == [(N - 1) * COMMITTEE, (N - 2) * COMMITTEE]
    assert sorted(launches["open"]) == [N - 2] * COMMITTEE + [N - 1] * COMMITTEE
    for run in (host, gpu):
        assert run.fields == {48} and run.kinds == KNOWN_CLIENT_MESSAGES and run.refused == []
        assert sorted(run.shared) == sorted((it, m) for it in (1, 2) for m in members)
        sums_hold(run, off)
    assert len(gpu.vectors) == len(host.vectors) == (N - 1) + (N - 2)
    for a, b in zip(host.vectors, gpu.vectors):
        assert a == b, (a[:2], b[:2])


def test_flipped_bit_silences_exactly_that_member(monkeypatch):
    members = committee()
    victim, dealer = members[4], [i for i in range(N) if i not in members][5]
    run = simulate(monkeypatch, True, tamper=flip_bit(1, victim, dealer))
    refused_exactly(run, members, 1, victim, dealer)


def test_replayed_share_of_the_iteration_before_is_refused(monkeypatch):
    """Red if the iteration is left out of the AAD."""
    members = committee()
    off = dropouts(members)
    victim, dealer = members[7], [i for i in range(N) if i not in members and i not in off][0]
    run = simulate(monkeypatch, True, offline=off, tamper=replay(2, victim, dealer))
    refused_exactly(run, members, 2, victim, dealer, off)


def test_field_of_another_length_is_a_failed_tag(monkeypatch, launches):
    members = committee()
    victim = members[2]
    d0, d1 = [i for i in range(N) if i not in members][:2]

    def cut(it, to, dealers, rows, history):
        if (it, to) == (1, victim):
            for d, keep in ((d0, 47), (d1, 32)):                      # truncated, tag cut off
                rows[dealers.index(d)] = (rows[dealers.index(d)][0][:keep], rows[dealers.index(d)][1])
        return rows

    run = simulate(monkeypatch, True, tamper=cut)
    assert run.refused == [(1, victim, sorted([d0, d1]))]
    assert N - 2 in launches["open"]                                   # the well-formed rows still went through the GPU
    sums_hold(run, None)


def test_too_few_members_left_and_the_server_raises(monkeypatch):
    from flamingo_amd.abides.flamingo import protocol
    members = committee()
    threshold = int(protocol.fraction * COMMITTEE)
    hit = set(members[:COMMITTEE - threshold + 1])                    # one more than the committee can lose
    dealer = [i for i in range(N) if i not in members][0]

    def tamper(it, to, dealers, rows, history):
        return flip_bit(1, to, dealer)(it, to, dealers, rows, history) if to in hit else rows

    with pytest.raises(RuntimeError, match="No enough shares"):
        simulate(monkeypatch, True, tamper=tamper)
