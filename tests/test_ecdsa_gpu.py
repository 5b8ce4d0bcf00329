"""flm_ecdsa_verify on the GPU against the CPU fixture (tests/golden/ecdsa_golden.json: plain-Python
FIPS 186-4 verdicts that OpenSSL's ECDSA_do_verify confirmed), verdict and flags, through the
host-pointer call and the *_dev call; batches around the wave size; the *_dev call's stream
contract; the engine's wrappers; and the agents with the committee's signature check switched on."""
from __future__ import annotations

import functools
import hashlib
import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 64


def _generator():
    spec = importlib.util.spec_from_file_location("make_ecdsa_golden",
                                                  os.path.join(ROOT, "tests", "golden", "make_ecdsa_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


G = _generator()
CASES = G.load()


def _rows(cases):
    hexrows = lambda k, n: np.frombuffer(b"".join(bytes.fromhex(c[k]) for c in cases), np.uint8).reshape(-1, n)  # noqa: E731
    sig = np.concatenate([hexrows("r", 32), hexrows("s", 32)], axis=1)
    return hexrows("q", 64).copy(), hexrows("e", 32).copy(), np.ascontiguousarray(sig)


@functools.lru_cache(maxsize=None)
def _pool():
    """16 signatures by plain Python and a tampered twin of each (a bit of r, s, e or Q in turn),
    valid and tampered alternating, with their plain-Python verdicts: computed once."""
    cases = []
    for i in range(16):
        d = G.h_int(f"pool-key:{i}") % (G.N - 1) + 1
        e = hashlib.sha256(f"pool message {i}".encode()).digest()
        cases += [G.signed_with_twins(f"pool{i}", d, e)[k] for k in (0, 1 + i % 4)]
    assert [c["ok"] for c in cases] == [True, False] * 16
    return tuple(cases)


@pytest.fixture(scope="module")
def eng():
    from flamingo_amd import MaskEngine
    e = MaskEngine(0)
    yield e
    e.close()


def _guarded(nbytes):
    """A device byte buffer of nbytes followed by GUARD bytes of 0xA5 -> (whole, payload view)."""
    import torch
    whole = torch.full((nbytes + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    return whole, whole[:nbytes]


def _guard_intact(whole):
    return bool((whole[-GUARD:] == 0xA5).all().item())


def _long_kernel(n=8192, reps=12):
    """Tens of ms of matmuls on the current stream (tests/test_streams_gpu.py) and their event."""
    import torch
    a = torch.ones((n, n), device="cuda")
    for _ in range(reps):
        a = a @ a * 1e-4
    ev = torch.cuda.Event()
    ev.record()
    return a, ev


def _dev_verify(eng, q, e, sig, with_flags=True):
    """the *_dev call on guarded outputs -> (ok, flags or None); the guards are checked here"""
    import torch
    n = q.shape[0]
    dq, de, ds = (torch.from_numpy(a).cuda() for a in (q, e, sig))
    ok_whole, ok = _guarded(n)
    fl_whole, fl_bytes = _guarded(4 * n)
    fl = fl_bytes.view(torch.int32)
    ok.fill_(7)
    fl.fill_(-1)
    eng.ecdsa_verify_dev(dq, de, ds, ok, fl if with_flags else None)
    torch.cuda.synchronize()
    assert _guard_intact(ok_whole) and _guard_intact(fl_whole)
    if not with_flags:
        assert bool((fl == -1).all().item()), "a NULL flags pointer must leave memory alone"
    return ok.cpu().numpy(), (fl.cpu().numpy().view(np.uint32) if with_flags else None)


def _mismatches(cases, ok, flags):
    return [(c["name"], c["ok"], c["flags"], int(o), int(f)) for c, o, f in zip(cases, ok, flags)
            if bool(o) != c["ok"] or int(f) != c["flags"]]


# ------------------------------------------------------------------ the fixture
def test_fixture_through_the_host_form(eng):
    ok, flags = eng.ecdsa_verify_wire(*_rows(CASES))
    assert ok.dtype == bool and flags.dtype == np.uint32
    assert _mismatches(CASES, ok, flags) == []


def test_fixture_through_the_dev_form(eng):
    ok, flags = _dev_verify(eng, *_rows(CASES))
    assert set(np.unique(ok)) <= {0, 1}
    assert _mismatches(CASES, ok, flags) == []


def test_fixture_cases_alone(eng):
    """each case as a batch of one: no neighbour's lanes beside it"""
    bad = []
    for c in CASES:
        ok, flags = eng.ecdsa_verify_wire(*_rows([c]))
        bad += _mismatches([c], ok, flags)
    assert bad == []


# ------------------------------------------------------------------ batch edges
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257])
def test_batch_edges(eng, n):
    cases = [_pool()[(i + 2 * (i // 32)) % 32] for i in range(n)]     # valid and tampered alternate in every wave
    q, e, sig = _rows(cases) if n else (np.zeros((0, 64), np.uint8), np.zeros((0, 32), np.uint8),
                                        np.zeros((0, 64), np.uint8))
    ok, flags = eng.ecdsa_verify_wire(q, e, sig)
    assert ok.shape == (n,) and flags.shape == (n,)
    assert _mismatches(cases, ok, flags) == []
    if n:
        assert int(ok.sum()) == (n + 1) // 2
    ok_d, flags_d = _dev_verify(eng, q, e, sig)
    assert _mismatches(cases, ok_d, flags_d) == []


# ------------------------------------------------------------------ the *_dev form
def test_dev_form_accepts_null_flags(eng):
    cases = list(_pool()[:5]) + [c for c in CASES if c["flags"]][:3]
    ok, none = _dev_verify(eng, *_rows(cases), with_flags=False)
    assert none is None
    assert [bool(o) for o in ok] == [c["ok"] for c in cases]


def test_dev_form_does_not_block(eng):
    import torch
    cases = [_pool()[i % 32] for i in range(65)]
    dq, de, ds = (torch.from_numpy(a).cuda() for a in _rows(cases))
    ok = torch.zeros(65, dtype=torch.uint8, device="cuda")
    fl = torch.zeros(65, dtype=torch.int32, device="cuda")
    eng.ecdsa_verify_dev(dq, de, ds, ok, fl)             # warm: the code object is loaded
    torch.cuda.synchronize()
    ok.zero_()
    _, busy = _long_kernel()
    eng.ecdsa_verify_dev(dq, de, ds, ok, fl)
    assert not busy.query(), "flm_ecdsa_verify_dev waited for earlier work on its stream"
    torch.cuda.synchronize()
    assert [bool(o) for o in ok.cpu().numpy()] == [c["ok"] for c in cases]


def test_argument_errors(eng):
    import ctypes
    import torch
    FLM_EINVAL = -1                   # include/flamingo_hip.h
    z = lambda *s: torch.zeros(s, dtype=torch.uint8, device="cuda")  # noqa: E731
    assert eng.lib.flm_ecdsa_verify(eng.ctx, None, None, None, 0, None, None) == 0          # n = 0: nothing read
    assert eng.lib.flm_ecdsa_verify(eng.ctx, None, None, None, -1, None, None) == FLM_EINVAL
    assert eng.lib.flm_ecdsa_verify(eng.ctx, None, None, None, (1 << 26) + 1, None, None) == FLM_EINVAL
    vp = ctypes.c_void_p
    assert eng.lib.flm_ecdsa_verify_dev(eng.ctx, vp(), vp(), vp(), 0, vp(), vp(), vp()) == 0
    assert eng.lib.flm_ecdsa_verify_dev(eng.ctx, vp(), vp(), vp(), -5, vp(), vp(), vp()) == FLM_EINVAL
    q = z(2 * 64 + 16)
    with pytest.raises(RuntimeError, match="16-byte aligned"):
        eng.ecdsa_verify_dev(q[1:129].view(2, 64), z(2, 32), z(2, 64), z(2))
    with pytest.raises(RuntimeError, match="NULL argument"):
        eng._check(eng.lib.flm_ecdsa_verify_dev(eng.ctx, vp(q.data_ptr()), vp(), vp(q.data_ptr()), 2, vp(q.data_ptr()),
                                                vp(), vp()), "flm_ecdsa_verify_dev")
    with pytest.raises(RuntimeError, match="2 keys for 2 digests and 3 signatures"):
        eng.ecdsa_verify_wire(np.zeros((2, 64), np.uint8), np.zeros((2, 32), np.uint8), np.zeros((3, 64), np.uint8))
    with pytest.raises(RuntimeError, match="must be"):
        eng.ecdsa_verify_wire(np.zeros((2, 63), np.uint8), np.zeros((2, 32), np.uint8), np.zeros((2, 64), np.uint8))
    torch.cuda.synchronize()


# ------------------------------------------------------------------ the engine's wrappers
def test_engine_verifies_openssl_signatures(eng):
    """ecdsa_verify hashes the messages itself and answers as crypto.ecdsa_verify does row by row"""
    from flamingo_amd import crypto as C
    keys = [C.keygen(bytes([i])) for i in range(6)]
    msgs = [f"offline set {i}".encode() * (i + 1) for i in range(6)]
    sigs = [C.ecdsa_sign(d, Q, m) for (d, Q), m in zip(keys, msgs)]
    pubs = [Q for _, Q in keys]
    assert eng.ecdsa_verify(pubs, msgs, sigs) == [True] * 6
    pubs2 = [pubs[1], pubs[1], None, pubs[3], (pubs[4][0], pubs[4][1] ^ 1), pubs[5], (1 << 256, 5)]
    msgs2 = [msgs[0], msgs[1] + b"!", msgs[2], msgs[3], msgs[4], msgs[5], msgs[0]]
    sigs2 = [sigs[0], sigs[1], sigs[2], sigs[3][:63], sigs[4], sigs[5], sigs[0]]
    got = eng.ecdsa_verify(pubs2, msgs2, sigs2)
    assert got == [False, False, False, False, False, True, False]
    want = [C.ecdsa_verify(p, m, s) if p is not None and len(s) == 64 and p[0] < (1 << 256) else False
            for p, m, s in zip(pubs2, msgs2, sigs2)]
    assert got == want
    assert eng.ecdsa_verify([], [], []) == []


def test_reference_side_binding(monkeypatch):
    """integration/util_flm.py's ecdsa_verify, called with the reference's types: EccPoint-like keys
    (.x, .y), the signed bytes, 64-byte signatures"""
    from types import SimpleNamespace
    from flamingo_amd import crypto as C
    monkeypatch.setenv("FLM_LIB", os.path.join(ROOT, "flamingo_amd", "lib", "libflamingo_hip.so"))
    spec = importlib.util.spec_from_file_location("util_flm", os.path.join(ROOT, "integration", "util_flm.py"))
    flm = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(flm)
    keys = [C.keygen(b"ref%d" % i) for i in range(5)]
    pts = [SimpleNamespace(x=Q[0], y=Q[1]) for _, Q in keys]
    msgs = [b"[3, 77, 100]", b"[]", b"x" * 200, b"[1]", b"[2]"]
    sigs = [C.ecdsa_sign(d, Q, m) for (d, Q), m in zip(keys, msgs)]
    assert flm.ecdsa_verify(pts, msgs, sigs) == [True] * 5
    assert flm.ecdsa_verify(pts, [msgs[0], b"[ ]"] + msgs[2:], sigs[:3] + [sigs[4], sigs[3][:60]]) == \
        [True, False, True, False, False]
    assert flm.ecdsa_verify([], [], []) == []


# ------------------------------------------------------------------ the agents
ROOT_SEED = "7e" * 32


def _run(check: bool, extra=()):
    """N = 128, L = 1024, 2 iterations, a committee of 10, three clients outside it offline"""
    from flamingo_amd.abides import config_flamingo as CF
    from flamingo_amd.abides.flamingo import protocol
    protocol.configure(root=bytes.fromhex(ROOT_SEED), committee=10)
    members = protocol.committee(128)
    offline = [i for i in range(128) if i not in members][:3]
    try:
        return CF.run(["-c", "flamingo", "-n", "128", "-i", "2", "-s", "11", "-k", "--offline",
                       ",".join(str(i) for i in offline), "--root_seed_hex", ROOT_SEED,
                       "--vector_len", "1024", "--committee_size", "10", "--latency", "deterministic"]
                      + (["--check_signatures", "--gpu_verify"] if check else []) + list(extra))
    finally:
        protocol.configure(check_signatures=False, gpu_verify=False)


def test_agents_check_signatures_on_the_gpu(monkeypatch):
    """N = 128 with dropouts, --check_signatures --gpu_verify: every committee member verifies its
    DEC's signatures in one MaskEngine.ecdsa_verify call (server + 10 members), all pass, and the sums
    are those of a run with the check off."""
    from flamingo_amd.engine import MaskEngine
    calls = []
    real = MaskEngine.ecdsa_verify

    def counted(self, pubs, msgs, sigs):
        out = real(self, pubs, msgs, sigs)
        calls.append((len(pubs), sum(out)))
        return out

    monkeypatch.setattr(MaskEngine, "ecdsa_verify", counted)
    off = _run(False)["server"]
    assert calls == []
    on = _run(True)["server"]
    assert calls == [(11, 11)] * 20                      # 10 members x 2 iterations
    assert sorted(on.results) == [1, 2]
    for it in (1, 2):
        assert on.online_counts[it] == 125 and np.all(on.results[it] == 125)
        assert np.array_equal(on.results[it], off.results[it])


def test_agents_equivocating_server_is_refused_by_that_member(monkeypatch):
    """The server shows committee member `victim` another offline set (with a genuine signature of
    its own over it): that member's payload differs from everyone else's, so it counts one valid
    entry, refuses, and the other members go on."""
    import json
    from flamingo_amd import crypto as C
    from flamingo_amd.abides.flamingo import protocol
    from flamingo_amd.abides.flamingo.client_agent import SA_ClientAgent
    from flamingo_amd.abides.flamingo.service_agent import SA_ServiceAgent
    victim = None                     # the fifth committee member, known once the run has a committee
    refused, shared = [], []
    orig_send = SA_ServiceAgent.sendMessage
    orig_client_send = SA_ClientAgent.sendMessage

    def lie(self, recipient, msg, *a, **kw):
        nonlocal victim
        if victim is None:
            victim = sorted(self.user_committee)[4]
        if msg.body["msg"] == "SIGN" and recipient == victim:
            pki = protocol.pki(self.num_clients)
            labels = json.dumps([1, 2, 3, 4]).encode()
            msg.body = dict(msg.body, labels=(labels, C.ecdsa_sign(pki.server_sk, pki.server_pk, labels)))
        return orig_send(self, recipient, msg, *a, **kw)

    def record(self, recipient, msg, *a, **kw):
        if msg.body["msg"] == "SIG_CHECK_FAILED":
            refused.append((msg.body["iteration"], msg.body["sender"], msg.body["valid"], msg.body["needed"]))
        elif msg.body["msg"] == "SHARED_RESULT":
            shared.append((msg.body["iteration"], msg.body["sender"]))
        return orig_client_send(self, recipient, msg, *a, **kw)

    monkeypatch.setattr(SA_ServiceAgent, "sendMessage", lie)
    monkeypatch.setattr(SA_ClientAgent, "sendMessage", record)
    srv = _run(True)["server"]
    assert refused == [(1, victim, 1, 7), (2, victim, 1, 7)]          # ceil(2/3 x 10) = 7
    assert len(shared) == 18 and victim not in {s for _, s in shared}
    for it in (1, 2):
        assert np.all(srv.results[it] == 125)                           # 9 shares >= the threshold
