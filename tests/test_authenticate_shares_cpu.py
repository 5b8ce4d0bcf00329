"""protocol.configure(authenticate_shares=True) on the oracle engine double, which has no dealing or
sealing calls, so the clients seal and the members open row by row on the host (crypto.aes_gcm_seal /
aes_gcm_open): the option off changes nothing; on, the shares carry their tag, an honest run still
sums to |U|, and a server that flips a bit of a sealed share, or replays last iteration's, gets
TAG_CHECK_FAILED from exactly the member it tried it on.  tests/test_authenticate_shares_gpu.py runs
the same scenarios (simulate, the tamper functions) on the real engine."""
from __future__ import annotations

import types

import numpy as np
import pytest

ROOT_SEED = "7e" * 32
N, L, COMMITTEE, ITERATIONS = 64, 64, 10, 2
KNOWN_CLIENT_MESSAGES = {"VECTOR", "SIGN", "SHARED_RESULT"}


@pytest.fixture
def oracle_engine(monkeypatch):
    from flamingo_amd.abides.flamingo import protocol
    from test_abides_protocol_cpu import OracleEngine
    monkeypatch.setattr(protocol, "_engine", OracleEngine())
    yield
    protocol.configure(committee=60, authenticate_shares=False, gpu_deal=True)


def committee():
    from flamingo_amd.abides.flamingo import protocol
    protocol.configure(root=bytes.fromhex(ROOT_SEED), committee=COMMITTEE)
    return sorted(protocol.committee(N))


def dropouts(members) -> dict:
    """two clients off the committee: one offline in both iterations, one in the second"""
    a, b = [i for i in range(N) if i not in members][:2]
    return {a: {1, 2}, b: {2}}


def simulate(monkeypatch, auth, gpu_deal=None, offline=None, tamper=None):
    """N = 64, L = 64, committee of 10, two iterations.  tamper(iteration, member, dealers, rows,
    history) -> rows rewrites the (ciphertext field, nonce) rows the server double hands `member` in
    SIGN; history[(iteration, member)] = (dealers, rows) as the honest server would have sent them.
    Returns .server, .vectors [(iteration, sender, enc_mi_shares text)], .fields {length of a
    ciphertext field}, .refused [(iteration, sender, bad)], .shared [(iteration, sender)], .kinds
    {message types the clients sent}."""
    from flamingo_amd.abides import config_flamingo as CF
    from flamingo_amd.abides.flamingo import protocol, wire
    from flamingo_amd.abides.flamingo.client_agent import SA_ClientAgent
    from flamingo_amd.abides.flamingo.service_agent import SA_ServiceAgent
    out = types.SimpleNamespace(vectors=[], fields=set(), refused=[], shared=[], kinds=set(), server=None)
    history = {}
    srv_send, clt_send = SA_ServiceAgent.sendMessage, SA_ClientAgent.sendMessage

    def server_send(self, recipient, msg, *a, **kw):
        b = msg.body
        if b["msg"] == "SIGN":
            dealers, rows = list(b["client_id_list"]), wire.deserialize_tuples_bytes(b["dec_target_mi"])
            history[(b["iteration"], recipient)] = (dealers, rows)
            if tamper is not None:
                new = tamper(b["iteration"], recipient, dealers, list(rows), history)
                msg.body = dict(b, dec_target_mi=wire.serialize_tuples_bytes(new))
        return srv_send(self, recipient, msg, *a, **kw)

    def client_send(self, recipient, msg, *a, **kw):
        b = msg.body
        out.kinds.add(b["msg"])
        if b["msg"] == "VECTOR":
            out.vectors.append((b["iteration"], b["sender"], b["enc_mi_shares"]))
            out.fields |= {len(ct) for ct, _ in wire.deserialize_tuples_bytes(b["enc_mi_shares"])}
        elif b["msg"] == "TAG_CHECK_FAILED":
            assert set(b) == {"msg", "iteration", "sender", "bad"} and kw.get("tag") == "tag_check_failed"
            out.refused.append((b["iteration"], b["sender"], list(b["bad"])))
        elif b["msg"] == "SHARED_RESULT":
            out.shared.append((b["iteration"], b["sender"]))
        return clt_send(self, recipient, msg, *a, **kw)

    with monkeypatch.context() as mp:
        mp.setattr(SA_ServiceAgent, "sendMessage", server_send)
        mp.setattr(SA_ClientAgent, "sendMessage", client_send)
        if offline:
            mp.setattr(CF, "offline_schedule", lambda n, its, always=(), dropout=0.0: {k: set(v) for k, v in offline.items()})
        argv = ["-c", "flamingo", "-n", str(N), "-i", str(ITERATIONS), "-s", "9", "-k", "--vector_len", str(L),
                "--committee_size", str(COMMITTEE), "--root_seed_hex", ROOT_SEED, "--latency", "deterministic"]
        if auth:
            argv += ["--authenticate_shares"]
        if gpu_deal is not None:
            protocol.configure(gpu_deal=gpu_deal)
        try:
            out.server = CF.run(argv)["server"]
        finally:
            protocol.configure(authenticate_shares=False, gpu_deal=True)
    return out


def flip_bit(iteration, member, dealer, byte=3):
    """the server flips one bit of `dealer`'s sealed share for `member` in `iteration`"""
    def tamper(it, to, dealers, rows, history):
        if (it, to) == (iteration, member):
            k = dealers.index(dealer)
            ct, nonce = rows[k]
            rows[k] = (ct[:byte] + bytes([ct[byte] ^ 0x10]) + ct[byte + 1:], nonce)
        return rows
    return tamper


def replay(iteration, member, dealer):
    """the server hands `member` the ciphertext `dealer` sealed for it in the iteration before"""
    def tamper(it, to, dealers, rows, history):
        if (it, to) == (iteration, member):
            old_dealers, old_rows = history[(iteration - 1, member)]
            rows[dealers.index(dealer)] = old_rows[old_dealers.index(dealer)]
            assert rows[dealers.index(dealer)] != history[(it, to)][1][dealers.index(dealer)]
        return rows
    return tamper


def sums_hold(run, offline):
    want = {it: N - sum(1 for its in (offline or {}).values() if it in its) for it in range(1, ITERATIONS + 1)}
    assert dict(run.server.online_counts) == want
    for it, n_on in want.items():
        assert np.all(np.asarray(run.server.results[it]) == n_on), it       # final_sum == |U| in every slot


def refused_exactly(run, members, iteration, victim, dealer, offline=None):
    """`victim` said TAG_CHECK_FAILED naming `dealer` in `iteration` and sent no shares then; every
    other member, and the victim in the other iteration, sent theirs; the sums still hold"""
    assert run.refused == [(iteration, victim, [dealer])]
    assert sorted(run.shared) == sorted((it, m) for it in range(1, ITERATIONS + 1) for m in members
                                        if (it, m) != (iteration, victim))
    sums_hold(run, offline)


# ------------------------------------------------------------------ the switch
def test_configure_takes_the_switch():
    """Fails on a tree without the feature: configure() has no authenticate_shares there."""
    from flamingo_amd.abides.flamingo import protocol
    from flamingo_amd.abides.config_flamingo import parse
    try:
        assert protocol.authenticate_shares_on() is False                    # off by default
        protocol.configure(authenticate_shares=True)
        assert protocol.authenticate_shares_on() is True
        protocol.configure()                                                 # a plain reset keeps the switch
        assert protocol.authenticate_shares_on() is True
    finally:
        protocol.configure(authenticate_shares=False)
    assert protocol.authenticate_shares_on() is False
    assert parse(["-c", "flamingo"])[1].authenticate_shares is False
    assert parse(["-c", "flamingo", "--authenticate_shares"])[1].authenticate_shares is True
    aad = protocol.share_aad(2, 0x01020304, 7)
    assert aad == bytes([0, 0, 0, 0, 0, 0, 0, 2, 1, 2, 3, 4, 0, 0, 0, 7])
    assert len({protocol.share_aad(*t) for t in ((1, 2, 3), (2, 2, 3), (1, 3, 2), (1, 2, 4))}) == 4


# ------------------------------------------------------------------ honest runs
def test_option_off_sends_what_it_always_sent(oracle_engine, monkeypatch):
    members = committee()
    off = dropouts(members)
    run = simulate(monkeypatch, False, offline=off)
    assert run.fields == {32} and run.kinds == KNOWN_CLIENT_MESSAGES and run.refused == []
    sums_hold(run, off)


def test_option_on_seals_with_the_tag_and_sums_to_the_online_count(oracle_engine, monkeypatch):
    from flamingo_amd.abides.flamingo import wire
    members = committee()
    off = dropouts(members)
    plain = simulate(monkeypatch, False, offline=off)
    run = simulate(monkeypatch, True, offline=off)
    assert run.fields == {48} and run.kinds == KNOWN_CLIENT_MESSAGES and run.refused == []
    assert sorted(run.shared) == sorted((it, m) for it in (1, 2) for m in members)
    sums_hold(run, off)
    # no new random draw: the same nonces, and the ciphertext is the old one with the tag behind it
    assert [(v[0], v[1]) for v in run.vectors] == [(v[0], v[1]) for v in plain.vectors]
    for (_, _, a), (_, _, b) in zip(plain.vectors, run.vectors):
        assert [(ct[:32], nonce) for ct, nonce in wire.deserialize_tuples_bytes(b)] == wire.deserialize_tuples_bytes(a)
    assert np.array_equal(run.server.results[1], plain.server.results[1])


# ------------------------------------------------------------------ a server that tampers
def test_flipped_bit_silences_exactly_that_member(oracle_engine, monkeypatch):
    members = committee()
    victim, dealer = members[4], [i for i in range(N) if i not in members][5]
    run = simulate(monkeypatch, True, tamper=flip_bit(1, victim, dealer))
    refused_exactly(run, members, 1, victim, dealer)


@pytest.mark.parametrize("byte", [0, 31, 32, 47], ids=["ct0", "ct31", "tag0", "tag15"])
def test_flipped_bit_anywhere_in_the_field(oracle_engine, monkeypatch, byte):
    members = committee()
    victim, dealer = members[0], members[1]                       # a dealer that sits on the committee itself
    run = simulate(monkeypatch, True, tamper=flip_bit(2, victim, dealer, byte))
    refused_exactly(run, members, 2, victim, dealer)


def test_replayed_share_of_the_iteration_before_is_refused(oracle_engine, monkeypatch):
    """Red if the iteration is left out of the AAD: the pair key is static, so the old ciphertext
    and tag would verify under it."""
    members = committee()
    off = dropouts(members)
    victim, dealer = members[7], [i for i in range(N) if i not in members and i not in off][0]
    run = simulate(monkeypatch, True, offline=off, tamper=replay(2, victim, dealer))
    refused_exactly(run, members, 2, victim, dealer, off)


def test_share_sealed_for_another_member_or_dealer_is_refused(oracle_engine, monkeypatch):
    """the other two parts of the AAD: rows swapped between two dealers fail for both"""
    members = committee()
    victim = members[3]
    d0, d1 = [i for i in range(N) if i not in members][:2]

    def swap(it, to, dealers, rows, history):
        if (it, to) == (1, victim):
            i, j = dealers.index(d0), dealers.index(d1)
            rows[i], rows[j] = rows[j], rows[i]
        return rows

    run = simulate(monkeypatch, True, tamper=swap)
    assert run.refused == [(1, victim, sorted([d0, d1]))]
    sums_hold(run, None)


def test_field_of_another_length_is_a_failed_tag(oracle_engine, monkeypatch):
    members = committee()
    victim = members[2]
    d0, d1, d2 = [i for i in range(N) if i not in members][:3]

    def cut(it, to, dealers, rows, history):
        if (it, to) == (1, victim):
            for d, keep in ((d0, 47), (d1, 32), (d2, 0)):              # truncated, tag cut off, empty
                rows[dealers.index(d)] = (rows[dealers.index(d)][0][:keep], rows[dealers.index(d)][1])
        return rows

    run = simulate(monkeypatch, True, tamper=cut)
    assert run.refused == [(1, victim, sorted([d0, d1, d2]))]
    sums_hold(run, None)


def test_too_few_members_left_and_the_server_raises(oracle_engine, monkeypatch):
    from flamingo_amd.abides.flamingo import protocol
    members = committee()
    threshold = int(protocol.fraction * COMMITTEE)
    assert 1 <= threshold < COMMITTEE
    hit = set(members[:COMMITTEE - threshold + 1])                   # one more than the committee can lose
    dealer = [i for i in range(N) if i not in members][0]

    def tamper(it, to, dealers, rows, history):
        return flip_bit(1, to, dealer)(it, to, dealers, rows, history) if to in hit else rows

    with pytest.raises(RuntimeError, match="No enough shares"):
        simulate(monkeypatch, True, tamper=tamper)
