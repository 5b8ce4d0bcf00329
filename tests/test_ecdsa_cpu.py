"""The CPU side of the ECDSA verification: the fixture regenerates to the same cases (plain Python
against OpenSSL), the kernel's constants and scalar recoding against their Python models, the
argument rules through the stand-alone checker, and the agents' signature check on the oracle
engine double (which has no ecdsa_verify, so the members verify row by row on the host)."""
from __future__ import annotations

import importlib.util
import math
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import ec_oracle as E  # noqa: E402


def _generator():
    spec = importlib.util.spec_from_file_location("make_ecdsa_golden",
                                                  os.path.join(ROOT, "tests", "golden", "make_ecdsa_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


G = _generator()


# ------------------------------------------------------------------ the fixture
def test_fixture_regenerates_and_openssl_agrees():
    cases = G.build()
    assert cases == G.load()
    assert G.check_against_openssl(cases) == len(cases) > 80
    by = {c["name"]: c for c in cases}
    assert os.path.getsize(G.OUT) < 64 * 1024
    # every kind of case the kernel must tell apart is there, with the verdict it must give
    assert by["the-other-s"]["ok"] and by["digest-zero"]["ok"] and by["digest-ff"]["ok"] and by["digest-plus-n"]["ok"]
    for nm in ("r-zero", "s-zero", "r-is-n", "s-is-n", "r-top"):
        assert (by[nm]["ok"], by[nm]["flags"]) == (False, 1), nm
    for nm in ("q-zero-bytes", "q-x-is-p", "q-x-top", "q-y-is-p-plus"):
        assert (by[nm]["ok"], by[nm]["flags"]) == (False, 2), nm
    assert by["q-zero-and-r-zero"]["flags"] == 3
    assert by["xR-above-n"]["ok"] and not by["xR-above-n/r-is-x"]["ok"]
    assert (by["sum-at-infinity"]["ok"], by["sum-at-infinity"]["flags"]) == (False, 4)
    assert by["u1G-equals-u2Q"]["ok"] and not by["u1G-equals-u2Q/r-bit"]["ok"]
    for nm in ("key-1", "key-2", "key-3", "key-n-minus-1", "key-n-minus-2"):
        assert by[nm]["ok"] and not by[nm + "/s-bit"]["ok"], nm


def test_crypto_verify_digest_is_openssl_on_the_digest():
    from flamingo_amd import crypto as C
    import hashlib
    d, Q = C.keygen(b"digest-level")
    sig = C.ecdsa_sign(d, Q, b"offline set")
    dg = hashlib.sha256(b"offline set").digest()
    assert C.ecdsa_verify_digest(Q, dg, sig) and C.ecdsa_verify(Q, b"offline set", sig)
    assert not C.ecdsa_verify_digest(Q, bytes(32), sig) and not C.ecdsa_verify_digest(None, dg, sig)
    assert not C.ecdsa_verify((Q[0], Q[1] ^ 1), b"offline set", sig)          # off the curve: no verdict but "no"
    assert not C.ecdsa_verify_digest(Q, dg, sig[:63])


# ------------------------------------------------------------------ the kernel's constants and models
def _hip_source() -> str:
    """flm_p256.hip (kGOdd) with the headers of its layers (kN0 is in flm_fe256.h)"""
    src = ""
    for name in ("flm_p256.hip", "flm_fe256.h", "flm_jac256.h"):
        with open(os.path.join(ROOT, "flamingo_amd", "csrc", name)) as f:
            src += f.read()
    return src


def test_constant_table_of_g_is_the_oracles():
    """kGOdd[t] = (2t+1) G, affine, Montgomery form, eight little-endian 32-bit limbs per coordinate"""
    src = _hip_source()
    body = src[src.index("kGOdd[8][16] = {"):]
    body = body[:body.index("};")]
    words = [int(w, 16) for w in re.findall(r"0x([0-9a-f]{8})u", body)]
    assert len(words) == 8 * 16
    R = 1 << 256
    for t in range(8):
        x, y = E.mul(2 * t + 1)
        for c, v in enumerate((x * R % E.P, y * R % E.P)):
            limbs = words[16 * t + 8 * c: 16 * t + 8 * c + 8]
            assert sum(w << (32 * i) for i, w in enumerate(limbs)) == v, (t, c)
    m = re.search(r"kN0 = 0x([0-9a-f]{8})u", src)
    assert (int(m.group(1), 16) & 0x3FFFFFFF) == (-pow(E.N, -1, 1 << 30)) % (1 << 30)     # kNInv30


def regular_digits(k: int):
    """the kernel's recoding (regular_recode / regular_next) of a scalar k < n: (sign, digits from
    the top), k = sign x (2^256 + sum d_i 16^i)"""
    neg = k % 2 == 0
    k = E.N - k if neg else k
    h = k >> 1
    digs = []
    for _ in range(64):
        digs.append(2 * (h >> 252) - 15)
        h = (h << 4) & ((1 << 256) - 1)
    return (-1 if neg else 1), digs


def test_regular_recoding_model():
    rng = np.random.default_rng(3)
    ks = [0, 1, 2, 3, 15, 16, 17, E.N - 1, E.N - 2, E.N - 3, (E.N - 1) // 2, 1 << 255, (1 << 255) + 1] + \
         [int.from_bytes(rng.bytes(32), "big") % E.N for _ in range(300)]
    for k in ks:
        sign, digs = regular_digits(k)
        assert len(digs) == 64 and all(d % 2 and -15 <= d <= 15 for d in digs)
        acc = 1
        for d in digs:
            acc = 16 * acc + d
        assert (sign * acc - k) % E.N == 0, k
        assert acc < (1 << 257)


def test_bingcd_schedule_inverts_mod_the_group_order():
    """inv_bingcd<kN, kNInv30>: the 18 x 30 schedule of tools/bingcd_model.py with the group order as
    the modulus converges and matches Fermat, on edge and random inputs"""
    import bingcd_model
    n, worst = bingcd_model.check(n_random=1500, seed=12, mod=E.N)
    assert n > 1500 and worst <= 18
    for x in (1, 2, E.N - 1, E.N - 2, 1 << 255, (1 << 64) - 1, (E.N + 1) // 2):
        assert bingcd_model.inv(x, mod=E.N) * x % E.N == 1


# ------------------------------------------------------------------ the argument rules
def test_argument_rules_checker(tmp_path):
    """tools/args_check.cpp (flm_call_args.h + the bounce-buffer layout), built without a sanitizer"""
    cxx = next((c for c in ("c++", "g++", "clang++", "hipcc") if shutil.which(c)), None)
    assert cxx, "no C++ compiler"
    exe = str(tmp_path / "args_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-I", os.path.join(ROOT, "flamingo_amd", "csrc"),
                    os.path.join(ROOT, "tools", "args_check.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "all checks passed" in out.stdout, out.stdout + out.stderr


def test_header_declares_and_library_binds_the_calls():
    from flamingo_amd import _lib
    with open(os.path.join(ROOT, "include", "flamingo_hip.h")) as f:
        hdr = f.read()
    for name in ("flm_ecdsa_verify", "flm_ecdsa_verify_dev"):
        assert re.search(r"\bint %s\(" % name, hdr) and name in _lib.SIGNATURES
    assert "SA_ClientAgent.py:387" in hdr and "SA_ServiceAgent.py:382-386" in hdr


# ------------------------------------------------------------------ the switches
def test_configure_takes_the_switches():
    """Fails on a tree without the feature: configure() has no check_signatures there."""
    from flamingo_amd.abides.flamingo import protocol
    try:
        assert protocol.check_signatures_on() is False          # off by default
        protocol.configure(check_signatures=True)
        assert protocol.check_signatures_on() is True
        protocol.configure()                                    # a plain reset keeps the switch, as gpu_deal
        assert protocol.check_signatures_on() is True
        protocol.configure(check_signatures=False, signature_quorum=0.5)
        assert protocol.check_signatures_on() is False and protocol.signatures_needed(60) == 30
        protocol.configure(signature_quorum=2 / 3)
        assert [protocol.signatures_needed(c) for c in (1, 3, 9, 10, 60)] == [1, 2, 6, 7, 40]
        assert all(protocol.signatures_needed(c) == math.ceil(2 * c / 3) for c in range(1, 200))
        with pytest.raises(ValueError):
            protocol.configure(signature_quorum=0)
    finally:
        protocol.configure(check_signatures=False, signature_quorum=2 / 3)
    from flamingo_amd.abides.config_flamingo import parse
    assert parse(["-c", "flamingo"])[1].check_signatures is False and parse(["-c", "flamingo"])[1].gpu_verify is False
    on = parse(["-c", "flamingo", "--check_signatures", "--gpu_verify"])[1]
    assert on.check_signatures is True and on.gpu_verify is True


# ------------------------------------------------------------------ the agents, host fallback
ROOT_SEED = "3c" * 32
COMMITTEE = 10


@pytest.fixture
def oracle_engine(monkeypatch):
    from flamingo_amd.abides.flamingo import protocol
    from test_abides_protocol_cpu import OracleEngine
    monkeypatch.setattr(protocol, "_engine", OracleEngine())
    yield
    protocol.configure(committee=60, check_signatures=False)


def _committee():
    from flamingo_amd.abides.flamingo import protocol
    protocol.configure(root=bytes.fromhex(ROOT_SEED), committee=COMMITTEE)
    return sorted(protocol.committee(128))


def _simulate(monkeypatch, check, offline=(), forged=(), equivocate_to=None):
    """N = 128, L = 64, one iteration on the oracle engine.  forged: members whose signature the server
    receives with a bit flipped; equivocate_to: the member the server shows another offline set.
    Returns (server, refusals [(sender, valid, needed)], senders of SHARED_RESULT, host verify calls)."""
    import json
    from flamingo_amd import crypto as C
    from flamingo_amd.abides import config_flamingo as CF
    from flamingo_amd.abides.flamingo import protocol
    from flamingo_amd.abides.flamingo.client_agent import SA_ClientAgent
    from flamingo_amd.abides.flamingo.service_agent import SA_ServiceAgent
    refused, shared, verified = [], [], []
    srv_recv, srv_send, clt_send, real_verify = (SA_ServiceAgent.receiveMessage, SA_ServiceAgent.sendMessage,
                                                 SA_ClientAgent.sendMessage, C.ecdsa_verify)

    def receive(self, t, msg):
        b = msg.body
        if b["msg"] == "SIGN" and b["sender"] in forged:
            payload, sig = b["signed_labels"]
            msg.body = dict(b, signed_labels=(payload, sig[:40] + bytes([sig[40] ^ 1]) + sig[41:]))
        return srv_recv(self, t, msg)

    def server_send(self, recipient, msg, *a, **kw):
        if msg.body["msg"] == "SIGN" and recipient == equivocate_to:
            pki = protocol.pki(self.num_clients)
            labels = json.dumps([1, 2, 3, 4]).encode()
            msg.body = dict(msg.body, labels=(labels, C.ecdsa_sign(pki.server_sk, pki.server_pk, labels)))
        return srv_send(self, recipient, msg, *a, **kw)

    def client_send(self, recipient, msg, *a, **kw):
        b = msg.body
        if b["msg"] == "SIG_CHECK_FAILED":
            assert set(b) == {"msg", "iteration", "sender", "valid", "needed"} and kw.get("tag") == "sig_check_failed"
            refused.append((b["sender"], b["valid"], b["needed"]))
        elif b["msg"] == "SHARED_RESULT":
            shared.append(b["sender"])
        return clt_send(self, recipient, msg, *a, **kw)

    with monkeypatch.context() as mp:
        mp.setattr(SA_ServiceAgent, "receiveMessage", receive)
        mp.setattr(SA_ServiceAgent, "sendMessage", server_send)
        mp.setattr(SA_ClientAgent, "sendMessage", client_send)
        mp.setattr(C, "ecdsa_verify", lambda *a: verified.append(1) or real_verify(*a))
        argv = ["-c", "flamingo", "-n", "128", "-i", "1", "-s", "5", "-k", "--vector_len", "64", "--committee_size",
                str(COMMITTEE), "--root_seed_hex", ROOT_SEED, "--latency", "deterministic"]
        if offline:
            argv += ["--offline", ",".join(str(i) for i in offline)]
        if check:
            argv += ["--check_signatures"]
        try:
            srv = CF.run(argv)["server"]
        finally:
            protocol.configure(check_signatures=False)
    return srv, refused, sorted(shared), len(verified)


@pytest.mark.parametrize("dropouts", [False, True], ids=["all_online", "dropouts"])
def test_honest_run_gives_the_same_sum_with_the_check_on(oracle_engine, monkeypatch, dropouts):
    members = _committee()
    offline = [i for i in range(128) if i not in members][:3] if dropouts else []
    off, r0, s0, v0 = _simulate(monkeypatch, False, offline)
    on, r1, s1, v1 = _simulate(monkeypatch, True, offline)
    assert v0 == 0 and r0 == [] and r1 == []
    assert v1 == COMMITTEE * (COMMITTEE + 1)                 # every member: the server's row + one per member
    assert s0 == s1 == members
    n_on = 128 - len(offline)
    assert on.online_counts == off.online_counts == {1: n_on}
    assert np.array_equal(on.results[1], off.results[1]) and np.all(on.results[1] == n_on)
    assert (len(on.recon_symbol) > 0) == dropouts


def test_one_forged_committee_signature_still_reaches_quorum(oracle_engine, monkeypatch):
    members = _committee()
    srv, refused, shared, _ = _simulate(monkeypatch, True, forged={members[2]})
    assert refused == [] and shared == members               # 9 of 10 verify, 7 needed
    assert np.all(srv.results[1] == 128)


def test_equivocating_server_is_refused_by_exactly_that_member(oracle_engine, monkeypatch):
    members = _committee()
    victim = members[6]
    srv, refused, shared, _ = _simulate(monkeypatch, True, equivocate_to=victim)
    assert refused == [(victim, 1, 7)]                       # only its own signature is over its payload
    assert shared == [m for m in members if m != victim]     # the others count 9: the victim's payload differs
    assert np.all(srv.results[1] == 128)                     # 9 decryptors >= the threshold


def test_below_quorum_every_member_refuses_and_the_server_raises(oracle_engine, monkeypatch):
    members = _committee()
    with pytest.raises(RuntimeError, match="No enough shares"):
        _simulate(monkeypatch, True, forged=set(members[:4]))       # 6 of 10 verify, 7 needed


def test_gpu_verify_switch_picks_the_engine_call(oracle_engine, monkeypatch):
    """verify_signatures: the host loop by default (a member's 61 rows are no faster on the GPU), the
    engine's batched call after configure(gpu_verify=True) -- where the engine has one"""
    from flamingo_amd import crypto as C
    from flamingo_amd.abides.flamingo import protocol
    from test_abides_protocol_cpu import OracleEngine
    d, Q = C.keygen(b"switch")
    rows = ([Q, Q, None], [b"a", b"b", b"a"], [C.ecdsa_sign(d, Q, b"a")] * 3)
    batches = []

    class WithBatch(OracleEngine):
        def ecdsa_verify(self, pubs, msgs, sigs):
            batches.append(len(pubs))
            return [p is not None and C.ecdsa_verify(p, m, s) for p, m, s in zip(pubs, msgs, sigs)]

    try:
        assert protocol.verify_signatures(*rows) == [True, False, False] and batches == []
        protocol.configure(gpu_verify=True)
        assert protocol.verify_signatures(*rows) == [True, False, False] and batches == []     # no such call: host
        monkeypatch.setattr(protocol, "_engine", WithBatch())
        assert protocol.verify_signatures(*rows) == [True, False, False] and batches == [3]
        protocol.configure(gpu_verify=False)
        assert protocol.verify_signatures(*rows) == [True, False, False] and batches == [3]
    finally:
        protocol.configure(gpu_verify=False)


def test_check_dec_signatures_counts_only_what_counts(oracle_engine):
    """signature good + sender on the committee + the member's own payload; malformed entries and
    a bad server signature are told apart"""
    from flamingo_amd import crypto as C
    from flamingo_amd.abides.flamingo import protocol
    members = _committee()
    pki = protocol.pki(128)
    outsider = next(i for i in range(128) if i not in members)
    labels = b"[5, 9]"
    server = (labels, C.ecdsa_sign(pki.server_sk, pki.server_pk, labels))
    mine, other = repr(server).encode(), b"another payload"
    sign = lambda i, p: (p, C.ecdsa_sign(pki.client_sk[i], pki.client_pk[i], p))  # noqa: E731
    dec = {members[0]: sign(members[0], mine), members[1]: sign(members[1], mine),
           members[2]: sign(members[2], other),                                  # good signature, other payload
           members[3]: (mine, sign(members[4], mine)[1]),                        # someone else's signature
           outsider: sign(outsider, mine),                                       # not on the committee
           members[5]: (mine, b"short"), members[6]: "junk", 4096: sign(members[0], mine), "7": sign(members[0], mine)}
    assert protocol.check_dec_signatures(128, server, dec, mine) == (True, 2, 7)
    assert protocol.check_dec_signatures(128, (b"[5]", server[1]), dec, mine) == (False, 2, 7)
    assert protocol.check_dec_signatures(128, None, {}, mine) == (False, 0, 7)
    assert protocol.check_dec_signatures(128, server, dec, None) == (True, 0, 7)
