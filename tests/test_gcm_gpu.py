"""flm_aes_gcm_seal and flm_aes_gcm_open on the GPU against the CPU fixture
(tests/golden/gcm_golden.json: OpenSSL AES-128-GCM, ciphertext and tag), bit for bit, through the
host-pointer calls, the *_dev calls and the reference-side binding; opening in place; guard bytes
behind every output; tampering with single rows of a 257-message batch; the error returns; and the
stream contract of the *_dev calls."""
from __future__ import annotations

import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 64
FLM_EINVAL = -1


def _generator():
    spec = importlib.util.spec_from_file_location("make_gcm_golden",
                                                  os.path.join(ROOT, "tests", "golden", "make_gcm_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


G = _generator()
FIX = G.load()["gcm"]
BY = {c["name"]: c for c in FIX}


def rows(case):
    """(keys, nonces, aad, data, ct, tags) as (n, width) uint8 arrays; ct and tags recomputed once"""
    n = case["n"]
    k, nc, a, d = (np.frombuffer(G.D.field_bytes(case[f]), np.uint8).reshape(n, -1) if case[w] else
                   np.zeros((n, 0), np.uint8)
                   for f, w in (("keys", "n"), ("nonces", "n"), ("aad", "aad_len"), ("data", "len")))
    ct, tags = G.expected(case)
    return (k, nc, a, d, np.frombuffer(ct, np.uint8).reshape(n, case["len"]), np.frombuffer(tags, np.uint8).reshape(n, 16))


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


def _cuda(*arrays):
    import torch
    return [torch.from_numpy(a.copy()).cuda() for a in arrays]


# ------------------------------------------------------------------ fixture, bit for bit
@pytest.mark.parametrize("case", FIX, ids=lambda c: c["name"])
def test_seal_and_open_match_fixture(eng, case):
    import torch
    n, ln = case["n"], case["len"]
    k, nc, a, d, want_ct, want_tags = rows(case)
    # host-pointer forms
    ct, tags = eng.aes_gcm_seal_wire(k, nc, d, aad=a)
    assert np.array_equal(ct, want_ct) and np.array_equal(tags, want_tags)
    plain, ok = eng.aes_gcm_open_wire(k, nc, want_ct, want_tags, aad=a)
    assert ok.all() and np.array_equal(plain, d)
    # device forms, every output behind a guard
    dk, dn, da, dd = _cuda(k, nc, a, d)
    w_ct, f_ct = _guarded(n * ln)
    w_tg, f_tg = _guarded(n * 16)
    w_ok, f_ok = _guarded(n)
    o_ct, o_tg = f_ct.view(n, ln), f_tg.view(n, 16)
    eng.aes_gcm_seal_dev(dk, dn, dd, o_tg, out=o_ct, aad=da)
    torch.cuda.synchronize()
    assert np.array_equal(o_ct.cpu().numpy(), want_ct) and np.array_equal(o_tg.cpu().numpy(), want_tags)
    assert np.array_equal(dd.cpu().numpy(), d)                                  # the input is left alone
    assert _guard_intact(w_ct) and _guard_intact(w_tg)
    # open in place (out == in), behind the guard: ciphertext -> plaintext
    f_ok.fill_(7)
    eng.aes_gcm_open_dev(dk, dn, o_ct, o_tg, f_ok, aad=da)
    torch.cuda.synchronize()
    assert (f_ok == 1).all().item() and np.array_equal(o_ct.cpu().numpy(), d)
    assert np.array_equal(o_tg.cpu().numpy(), want_tags)                        # open only reads the tags
    assert _guard_intact(w_ct) and _guard_intact(w_tg) and _guard_intact(w_ok)
    # seal in place: plaintext -> ciphertext
    eng.aes_gcm_seal_dev(dk, dn, o_ct, o_tg, aad=da)
    torch.cuda.synchronize()
    assert np.array_equal(o_ct.cpu().numpy(), want_ct) and np.array_equal(o_tg.cpu().numpy(), want_tags)
    assert _guard_intact(w_ct) and _guard_intact(w_tg)


def test_host_forms_in_place(eng):
    """in == out through the host-pointer calls: seal, then open, on one buffer"""
    from flamingo_amd._lib import p_u8
    case = BY["gcm_nonce16_aad20_len33_n65"]
    k, nc, a, d, want_ct, want_tags = (x.copy() for x in rows(case))
    buf, tags, ok = d.copy(), np.zeros((65, 16), np.uint8), np.full(65, 9, np.uint8)
    rc = eng.lib.flm_aes_gcm_seal(eng.ctx, p_u8(k), p_u8(nc), 16, p_u8(a), 20, p_u8(buf), p_u8(buf), 33, p_u8(tags), 65)
    assert rc == 0 and np.array_equal(buf, want_ct) and np.array_equal(tags, want_tags)
    rc = eng.lib.flm_aes_gcm_open(eng.ctx, p_u8(k), p_u8(nc), 16, p_u8(a), 20, p_u8(buf), p_u8(tags), p_u8(buf), 33,
                                  p_u8(ok), 65)
    assert rc == 0 and np.array_equal(buf, d) and (ok == 1).all()


def test_reference_side_binding(monkeypatch):
    """integration/util_flm.py's aes_gcm_seal and aes_gcm_open, called with the reference's types"""
    monkeypatch.setenv("FLM_LIB", os.path.join(ROOT, "flamingo_amd", "lib", "libflamingo_hip.so"))
    import torch  # noqa: F401  (one HIP runtime per process: torch's, loaded first)
    spec = importlib.util.spec_from_file_location("util_flm", os.path.join(ROOT, "integration", "util_flm.py"))
    flm = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(flm)
    for name in ("gcm_nonce16_aad16_len32_n65", "gcm_nonce12_aad0_len17_n65", "gcm_nonce16_aad20_len0_n65"):
        case = BY[name]
        k, nc, a, d, ct, tags = ([bytes(r) for r in x] for x in rows(case))
        aads = a if case["aad_len"] else None
        assert flm.aes_gcm_seal(k, nc, d, aads) == list(zip(ct, tags))
        assert flm.aes_gcm_open(k, nc, ct, tags, aads) == d
        bad = [tags[0][:5] + bytes([tags[0][5] ^ 4]) + tags[0][6:]] + tags[1:]
        assert flm.aes_gcm_open(k, nc, ct, bad, aads) == [None] + d[1:]
    assert flm.aes_gcm_seal([], [], []) == [] and flm.aes_gcm_open([], [], [], []) == []


# ------------------------------------------------------------------ tampering
TAMPER_ROWS = (0, 63, 64, 255, 256)
TAMPER_KINDS = ("ct0", "ct_last", "tag0", "tag15", "aad", "nonce", "key")


def _tampered(kind):
    """the 257-message batch, sealed, with one bit flipped in `kind` of each row of TAMPER_ROWS"""
    case = BY["gcm_nonce16_aad16_len32_n257"]
    k, nc, a, d, ct, tags = (x.copy() for x in rows(case))
    target, col = {"ct0": (ct, 0), "ct_last": (ct, 31), "tag0": (tags, 0), "tag15": (tags, 15), "aad": (a, 9),
                   "nonce": (nc, 15), "key": (k, 7)}[kind]
    for j, r in enumerate(TAMPER_ROWS):
        target[r, col] ^= np.uint8(1 << (j % 8))
    want_ok = np.ones(257, bool)
    want_ok[list(TAMPER_ROWS)] = False
    want = d.copy()
    want[~want_ok] = 0
    return k, nc, a, ct, tags, want, want_ok


@pytest.mark.parametrize("kind", TAMPER_KINDS)
def test_tampered_rows_fail_alone_and_come_back_zero(eng, kind):
    import torch
    k, nc, a, ct, tags, want, want_ok = _tampered(kind)
    plain, ok = eng.aes_gcm_open_wire(k, nc, ct, tags, aad=a)
    assert np.array_equal(ok, want_ok) and np.array_equal(plain, want)
    assert not plain[~want_ok].any() and plain[want_ok].any(axis=1).all()
    # the device form, in place: a failed row holds zeros, not its ciphertext and not its plaintext
    dk, dn, da, dt = _cuda(k, nc, a, tags)
    w_ct, f_ct = _guarded(257 * 32)
    w_ok, f_ok = _guarded(257)
    f_ct.copy_(torch.from_numpy(ct.copy()).view(-1))
    f_ok.fill_(7)
    eng.aes_gcm_open_dev(dk, dn, f_ct.view(257, 32), dt, f_ok, aad=da)
    torch.cuda.synchronize()
    assert np.array_equal(f_ok.cpu().numpy(), want_ok.astype(np.uint8))         # 0 or 1, nothing else
    assert np.array_equal(f_ct.view(257, 32).cpu().numpy(), want)
    assert _guard_intact(w_ct) and _guard_intact(w_ok)


# ------------------------------------------------------------------ error returns
def test_argument_errors_write_nothing(eng):
    import torch
    from flamingo_amd._lib import p_u8
    k, nc, a, d = (np.zeros((2, w), np.uint8) for w in (16, 16, 16, 32))
    out, tags, ok = (np.full(s, 0x5A, np.uint8) for s in ((2, 32), (2, 16), (2,)))
    lib, ctx = eng.lib, eng.ctx

    def seal(nl=16, aad=a, al=16, src=d, dst=out, ln=32, tg=tags, n=2, kk=k, nn=nc):
        p = lambda x: p_u8(x) if x is not None else None  # noqa: E731
        return lib.flm_aes_gcm_seal(ctx, p(kk), p(nn), nl, p(aad), al, p(src), p(dst), ln, p(tg), n)

    def open_(nl=16, aad=a, al=16, src=d, dst=out, ln=32, tg=tags, n=2, kk=k, nn=nc, okp=ok):
        p = lambda x: p_u8(x) if x is not None else None  # noqa: E731
        return lib.flm_aes_gcm_open(ctx, p(kk), p(nn), nl, p(aad), al, p(src), p(tg), p(dst), ln, p(okp), n)

    bad = [dict(nl=13), dict(nl=0), dict(nl=8), dict(ln=257), dict(al=65), dict(n=-1), dict(n=(1 << 26) + 1),
           dict(kk=None), dict(nn=None), dict(src=None), dict(dst=None), dict(tg=None),
           dict(aad=None), dict(al=0)]                      # aad_len without aad; aad without aad_len
    for f in (seal, open_):
        for kw in bad:
            assert f(**kw) == FLM_EINVAL, (f.__name__, kw)
            assert lib.flm_last_error(ctx)
    assert open_(okp=None) == FLM_EINVAL
    assert (out == 0x5A).all() and (tags == 0x5A).all() and (ok == 0x5A).all()
    # through the engine: the message names what is wrong
    with pytest.raises(RuntimeError, match="nonce_len must be 12 or 16"):
        eng.aes_gcm_seal_wire(k, np.zeros((2, 13), np.uint8), d)
    with pytest.raises(RuntimeError, match="len must be in 0..256"):
        eng.aes_gcm_open_wire(k, nc, np.zeros((2, 257), np.uint8), tags)
    with pytest.raises(RuntimeError, match="aad_len must be in 0..64"):
        eng.aes_gcm_seal_wire(k, nc, d, aad=np.zeros((2, 65), np.uint8))
    # the device forms refuse the same sizes before anything is enqueued
    z = lambda *s: torch.zeros(s, dtype=torch.uint8, device="cuda")  # noqa: E731
    g_tags, g_ok = torch.full((2, 16), 0x5A, dtype=torch.uint8, device="cuda"), torch.full((2,), 0x5A, dtype=torch.uint8,
                                                                                        device="cuda")
    with pytest.raises(RuntimeError, match="nonce_len must be 12 or 16"):
        eng.aes_gcm_seal_dev(z(2, 16), z(2, 13), z(2, 32), g_tags)
    with pytest.raises(RuntimeError, match="len must be in 0..256"):
        eng.aes_gcm_open_dev(z(2, 16), z(2, 16), z(2, 257), g_tags, g_ok)
    with pytest.raises(RuntimeError, match="aad_len must be in 0..64"):
        eng.aes_gcm_open_dev(z(2, 16), z(2, 16), z(2, 32), g_tags, g_ok, aad=z(2, 65))
    torch.cuda.synchronize()
    assert (g_tags == 0x5A).all().item() and (g_ok == 0x5A).all().item()


def test_empty_batch_and_empty_message_are_accepted(eng):
    import torch
    from flamingo_amd import crypto as C
    from flamingo_amd._lib import p_u8
    e = lambda w: np.zeros((0, w), np.uint8)  # noqa: E731
    ct, tags = eng.aes_gcm_seal_wire(e(16), e(12), e(32), aad=e(16))                        # n = 0
    assert ct.shape == (0, 32) and tags.shape == (0, 16)
    plain, ok = eng.aes_gcm_open_wire(e(16), e(16), e(32), e(16))
    assert plain.shape == (0, 32) and ok.shape == (0,)
    assert eng.lib.flm_aes_gcm_seal(eng.ctx, None, None, 16, None, 0, None, None, 32, None, 0) == 0
    assert eng.lib.flm_aes_gcm_open(eng.ctx, None, None, 16, None, 0, None, None, None, 32, None, 0) == 0
    z = lambda *s: torch.zeros(s, dtype=torch.uint8, device="cuda")  # noqa: E731
    eng.aes_gcm_seal_dev(z(0, 16), z(0, 16), z(0, 32), z(0, 16))
    eng.aes_gcm_open_dev(z(0, 16), z(0, 16), z(0, 32), z(0, 16), z(0))
    # len = 0: a tag over the AAD alone, in and out NULL
    k, nc, a = (np.frombuffer(G.D.prg("empty-" + s, 3 * w), np.uint8).reshape(3, w).copy()
                 for s, w in (("k", 16), ("n", 12), ("a", 20)))
    tags, ok = np.zeros((3, 16), np.uint8), np.full(3, 9, np.uint8)
    assert eng.lib.flm_aes_gcm_seal(eng.ctx, p_u8(k), p_u8(nc), 12, p_u8(a), 20, None, None, 0, p_u8(tags), 3) == 0
    assert [bytes(t) for t in tags] == [C.aes_gcm_seal(bytes(k[i]), b"", bytes(nc[i]), bytes(a[i]))[1] for i in range(3)]
    a[1, 19] ^= 0x80
    assert eng.lib.flm_aes_gcm_open(eng.ctx, p_u8(k), p_u8(nc), 12, p_u8(a), 20, None, p_u8(tags), None, 0, p_u8(ok), 3) == 0
    assert ok.tolist() == [1, 0, 1]
    dk, dn, da, dt = _cuda(k, nc, a, tags)
    d_ok = z(3)
    eng.aes_gcm_open_dev(dk, dn, z(3, 0), dt, d_ok, aad=da)
    torch.cuda.synchronize()
    assert d_ok.cpu().tolist() == [1, 0, 1]


# ------------------------------------------------------------------ stream contract
def test_seal_and_open_dev_do_not_block(eng):
    import torch
    case = BY["gcm_nonce16_aad16_len32_n65"]
    k, nc, a, d, want_ct, want_tags = rows(case)
    dk, dn, da, dd = _cuda(k, nc, a, d)
    ct, tags = torch.zeros((65, 32), dtype=torch.uint8, device="cuda"), torch.zeros((65, 16), dtype=torch.uint8, device="cuda")
    plain, ok = torch.zeros((65, 32), dtype=torch.uint8, device="cuda"), torch.zeros(65, dtype=torch.uint8, device="cuda")
    eng.aes_gcm_seal_dev(dk, dn, dd, tags, out=ct, aad=da)        # warm: the code objects are loaded
    eng.aes_gcm_open_dev(dk, dn, ct, tags, ok, out=plain, aad=da)
    torch.cuda.synchronize()
    for t in (ct, tags, plain, ok):
        t.zero_()
    _, busy = _long_kernel()
    eng.aes_gcm_seal_dev(dk, dn, dd, tags, out=ct, aad=da)
    eng.aes_gcm_open_dev(dk, dn, ct, tags, ok, out=plain, aad=da)
    assert not busy.query(), "flm_aes_gcm_seal_dev / flm_aes_gcm_open_dev waited for earlier work on the stream"
    torch.cuda.synchronize()
    assert np.array_equal(ct.cpu().numpy(), want_ct) and np.array_equal(tags.cpu().numpy(), want_tags)
    assert np.array_equal(plain.cpu().numpy(), d) and (ok == 1).all().item()
