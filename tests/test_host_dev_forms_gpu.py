"""The host-pointer form and the *_dev form of each batch crypto call are one computation: on the same
inputs flm_shamir_combine, flm_shamir_deal, flm_aes_gcm_xor / _seal / _open, flm_ecdsa_verify and
flm_feldman_verify return the same bytes through both, at one lane and one past a wave, with each
optional array present and absent; and a call either form refuses (a negative size, one over the
2^26 row limit, a NULL required array) is refused by both with the same code and the same
flm_last_error text, before any device work.  The alignment rule is the *_dev forms' own: the host
forms hand them the context's device buffers."""
from __future__ import annotations

import ctypes
import json
import os

import numpy as np
import pytest

import feldman_cases as F

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLM_EINVAL = -1                   # include/flamingo_hip.h
OVER = (1 << 26) + 1              # one over the row limit
FILL = 0x5C                       # what every output holds before a call
NS = (1, 65)


@pytest.fixture(scope="module")
def eng():
    from flamingo_amd import MaskEngine
    e = MaskEngine(0)
    yield e
    e.close()


class Arr:
    """An array argument of a call: a numpy array, or None for a NULL pointer."""
    def __init__(self, a, out=False):
        self.a, self.out = a, out


NULL = Arr(None)


def out(shape, dtype=np.uint8):
    return Arr(np.full(shape, FILL * (0x01010101 if dtype == np.uint32 else 1), dtype), out=True)


def _run(eng, name, args, form, off8=None):
    """One call of `name` (host form) or `name`_dev on torch's stream.  args: the C arguments after ctx
    in order, arrays as Arr; off8: index into args of an array handed over 8 bytes off a 16-byte
    boundary (dev form).  -> (return code, flm_last_error, the output arrays' bytes after the call)."""
    import torch
    from flamingo_amd._lib import p_u8, p_u32
    cargs, outs, alive = [], [], []                 # alive: the device arrays, until the call has run
    for i, v in enumerate(args):
        if not isinstance(v, Arr) or v.a is None:
            cargs.append(None if isinstance(v, Arr) else v)
            continue
        if form == "host":
            h = v.a.copy()
            cargs.append(p_u32(h) if h.dtype == np.uint32 else p_u8(h))
            fetch = h.tobytes
        else:
            raw = np.ascontiguousarray(v.a).view(np.uint8).reshape(-1)
            shift = 8 if i == off8 else 0
            t = torch.zeros(raw.size + 16, dtype=torch.uint8, device="cuda")
            assert t.data_ptr() % 16 == 0
            t[shift:shift + raw.size] = torch.from_numpy(raw.copy())
            cargs.append(ctypes.c_void_p(t.data_ptr() + shift))
            alive.append(t)
            fetch = lambda t=t, shift=shift, n=raw.size: t[shift:shift + n].cpu().numpy().tobytes()  # noqa: E731
        if v.out:
            outs.append(fetch)
    if form == "dev":
        cargs.append(eng._stream_handle(None))
    rc = getattr(eng.lib, name + ("_dev" if form == "dev" else ""))(eng.ctx, *cargs)
    err = eng.lib.flm_last_error(eng.ctx) if rc else b""
    if form == "dev":
        torch.cuda.synchronize()
    return rc, err, [f() for f in outs]


def _same(eng, name, args):
    """both forms accept the call and return the same bytes, none of them left as it was"""
    rc_h, _, got_h = _run(eng, name, args, "host")
    rc_d, _, got_d = _run(eng, name, args, "dev")
    assert rc_h == 0 and rc_d == 0
    assert got_h == got_d
    assert all(FILL.to_bytes(1, "big") * len(b) != b for b in got_h)
    return got_h


def _refused(eng, name, cases, misaligned=()):
    """each of `cases` (argument lists) is refused by both forms alike, outputs untouched; each
    (args, index) of `misaligned` by the *_dev form"""
    for args in cases:
        rc_h, err_h, got_h = _run(eng, name, args, "host")
        rc_d, err_d, got_d = _run(eng, name, args, "dev")
        assert rc_h == FLM_EINVAL and rc_d == FLM_EINVAL
        assert err_h == err_d and err_h
        assert all(set(b) <= {FILL} for b in got_h + got_d)
    for args, i in misaligned:
        rc, err, got = _run(eng, name, args, "dev", off8=i)
        assert rc == FLM_EINVAL and b"16-byte aligned" in err
        assert all(set(b) <= {FILL} for b in got)


def _rng(*key):
    return np.random.Generator(np.random.PCG64([20241, *key]))


def _bytes(g, *shape):
    return g.integers(0, 256, shape, dtype=np.uint8)


def _swap(args, i, v):
    a = list(args)
    a[i] = v
    return a


# ------------------------------------------------------------------ flm_shamir_combine
def _combine_args(M, T=2):
    g = _rng(1, M)
    return [Arr(_bytes(g, T, M, 32)), Arr(_bytes(g, T, 32)), T, M, out((M, 32))]


@pytest.mark.parametrize("M", NS)
def test_shamir_combine(eng, M):
    _same(eng, "flm_shamir_combine", _combine_args(M))


def test_shamir_combine_refusals(eng):
    a = _combine_args(1)
    _refused(eng, "flm_shamir_combine", [_swap(a, 3, -1), _swap(a, 3, (1 << 25) + 1), _swap(a, 0, NULL),
                                         _swap(a, 4, NULL)])


# ------------------------------------------------------------------ flm_shamir_deal
def _deal_args(M, T=2, C=2):
    g = _rng(2, M)
    return [Arr(_bytes(g, T, M, 32)), T, M, Arr(np.arange(1, C + 1, dtype=np.uint32)), C, out((C, M, 32))]


@pytest.mark.parametrize("M", NS)
def test_shamir_deal(eng, M):
    _same(eng, "flm_shamir_deal", _deal_args(M))


def test_shamir_deal_refusals(eng):
    a = _deal_args(1)
    _refused(eng, "flm_shamir_deal", [_swap(a, 2, -1), _swap(a, 2, (1 << 25) + 1), _swap(a, 3, NULL),
                                      _swap(a, 0, NULL)],
             misaligned=[(a, 0), (a, 5)])


# ------------------------------------------------------------------ flm_aes_gcm_xor / _seal / _open
def _gcm_rows(n, ln, al, nonce_len=12):
    g = _rng(3, n, ln, al)
    return (_bytes(g, n, 16), _bytes(g, n, nonce_len), _bytes(g, n, al) if al else None,
            _bytes(g, n, ln) if ln else None)


def _xor_args(n, ln):
    k, nc, _, d = _gcm_rows(n, ln, 0)
    return [Arr(k), Arr(nc), nc.shape[1], Arr(d), out((n, ln)), ln, n]


def _seal_args(n, ln, al):
    k, nc, a, d = _gcm_rows(n, ln, al)
    return [Arr(k), Arr(nc), nc.shape[1], Arr(a), al, Arr(d), out((n, ln)) if ln else NULL, ln, out((n, 16)), n]


def _open_args(n, ln, al, ct, tags):
    k, nc, a, _ = _gcm_rows(n, ln, al)
    return [Arr(k), Arr(nc), nc.shape[1], Arr(a), al, Arr(ct), Arr(tags), out((n, ln)) if ln else NULL, ln,
            out((n,)), n]


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("ln", (1, 17))
def test_aes_gcm_xor(eng, n, ln):
    _same(eng, "flm_aes_gcm_xor", _xor_args(n, ln))


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("ln,al", [(1, 0), (1, 1), (17, 0), (17, 1), (0, 1)])
def test_aes_gcm_seal_and_open(eng, n, ln, al):
    """len 0 (a tag over the AAD alone) leaves the data arrays out; open sees seal's rows, every other tag bent"""
    sealed = _same(eng, "flm_aes_gcm_seal", _seal_args(n, ln, al))
    ct = np.frombuffer(sealed[0], np.uint8).reshape(n, ln) if ln else None
    tags = np.frombuffer(sealed[-1], np.uint8).reshape(n, 16).copy()
    tags[1::2, 15] ^= 1
    opened = _same(eng, "flm_aes_gcm_open", _open_args(n, ln, al, ct, tags))
    ok = np.frombuffer(opened[-1], np.uint8)
    assert ok.tolist() == [1 - i % 2 for i in range(n)]
    if ln:
        plain = np.frombuffer(opened[0], np.uint8).reshape(n, ln)
        assert (plain[0::2] == _gcm_rows(n, ln, al)[3][0::2]).all() and not plain[1::2].any()


def test_aes_gcm_refusals(eng):
    x = _xor_args(1, 1)
    _refused(eng, "flm_aes_gcm_xor", [_swap(x, 6, -1), _swap(x, 6, OVER), _swap(x, 0, NULL), _swap(x, 4, NULL)])
    s = _seal_args(1, 1, 1)
    _refused(eng, "flm_aes_gcm_seal", [_swap(s, 9, -1), _swap(s, 9, OVER), _swap(s, 1, NULL), _swap(s, 3, NULL),
                                       _swap(s, 8, NULL)])
    o = _open_args(1, 1, 1, np.zeros((1, 1), np.uint8), np.zeros((1, 16), np.uint8))
    _refused(eng, "flm_aes_gcm_open", [_swap(o, 10, -1), _swap(o, 10, OVER), _swap(o, 6, NULL), _swap(o, 9, NULL)])


# ------------------------------------------------------------------ flm_ecdsa_verify
def _ecdsa_args(n, flags=True):
    """the first n rows of the fixture (tests/golden/ecdsa_golden.json): valid and refused signatures"""
    with open(os.path.join(ROOT, "tests", "golden", "ecdsa_golden.json")) as f:
        cases = json.load(f)["cases"][:n]
    rows = lambda *ks: np.frombuffer(b"".join(bytes.fromhex("".join(c[k] for k in ks)) for c in cases),  # noqa: E731
                                     np.uint8).reshape(n, -1).copy()
    return [Arr(rows("q")), Arr(rows("e")), Arr(rows("r", "s")), n, out((n,)),
            out((n,), np.uint32) if flags else NULL]


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("flags", (True, False), ids=("flags", "noflags"))
def test_ecdsa_verify(eng, n, flags):
    got = _same(eng, "flm_ecdsa_verify", _ecdsa_args(n, flags))
    assert got[0][0] == 1         # the fixture's first row verifies


def test_ecdsa_verify_refusals(eng):
    a = _ecdsa_args(1)
    _refused(eng, "flm_ecdsa_verify", [_swap(a, 3, -1), _swap(a, 3, OVER), _swap(a, 1, NULL), _swap(a, 4, NULL)],
             misaligned=[(a, 0), (a, 1), (a, 2)])


# ------------------------------------------------------------------ flm_feldman_verify
def _feldman_args(n, dealer=True, points=True, flags=True, T=2, M=2, x_bits=2):
    """two dealers' degree-1 polynomials; row i: dealer i % M at x = 1 + i % 3, every third share one off"""
    coeffs = [[0x1234567 + 11 * d, 0x89ABCDE + 7 * d] for d in range(M)]
    com = np.frombuffer(b"".join(F.commit([coeffs[d][k] for d in range(M)])[d] for k in range(T) for d in range(M)),
                        np.uint8).reshape(T, M, 64).copy()
    xs = np.array([1 + i % 3 for i in range(n)], np.uint32)
    sh = np.frombuffer(b"".join(((F.poly(coeffs[i % M], int(xs[i])) + (i % 3 == 2)) % F.N).to_bytes(32, "big")
                                for i in range(n)), np.uint8).reshape(n, 32).copy()
    return [Arr(com), T, M, Arr((np.arange(n) % M).astype(np.uint32) if dealer else None), Arr(xs), x_bits, Arr(sh), n,
            out((n,)), out((n, 64)) if points else NULL, out((n,), np.uint32) if flags else NULL]


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("opt", range(8), ids=lambda o: "".join(c if o >> i & 1 else "-" for i, c in enumerate("dpf")))
def test_feldman_verify(eng, n, opt):
    got = _same(eng, "flm_feldman_verify", _feldman_args(n, bool(opt & 1), bool(opt & 2), bool(opt & 4)))
    assert list(got[0]) == [int(i % 3 != 2) for i in range(n)]


def test_feldman_verify_refusals(eng):
    a = _feldman_args(1)
    _refused(eng, "flm_feldman_verify", [_swap(a, 7, -1), _swap(a, 7, OVER), _swap(a, 0, NULL), _swap(a, 4, NULL),
                                         _swap(a, 8, NULL)],
             misaligned=[(a, 0), (a, 6), (a, 9)])
