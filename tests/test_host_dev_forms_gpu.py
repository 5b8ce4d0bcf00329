"""The host-pointer form and the *_dev form of each batch crypto call are one computation: on the same
inputs flm_shamir_combine, flm_shamir_deal, flm_aes_gcm_xor / _seal / _open, flm_ecdsa_verify and
flm_feldman_verify return the same bytes through both, at one lane and one past a wave, with each
optional array present and absent; and a call either form refuses (a negative size, one over the
2^26 row limit, a NULL required array) is refused by both with the same code and the same
flm_last_error text, before any device work.  The alignment rule is the *_dev forms' own: the host
forms hand them the context's device buffers.

The round-path calls (flm_client_mask, flm_client_encode_mask, flm_decode_sum, flm_prg_expand, and
flm_mask_accumulate / flm_aggregate_unmask against flm_aggregate_unmask_dev) are held to the same: rows of
L words at L = 1 (below one 16-byte quad), 5 (a quad and a tail) and 1025 (one past the 1024-slot tile
and past four of the small kernel's 256-slot tiles), one client and three (one of them without seeds,
signs of both kinds).  Their seg and signs are host arrays in both forms, and their *_dev forms take
row pitches the host forms have no argument for: only the first L words of a row are compared."""
from __future__ import annotations

import ctypes
import json
import os

import numpy as np
import pytest

import codec_cases as C
import feldman_cases as F

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLM_EINVAL, FLM_ERANGE = -1, -4   # include/flamingo_hip.h
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
    """An array argument of a call: a numpy array, or None for a NULL pointer.  host: a host array in both
    forms; pitch: the *_dev form gets the rows of a 2-D array `pitch` elements apart (the host form packed)."""
    def __init__(self, a, out=False, host=False, pitch=None):
        self.a, self.out, self.host, self.pitch = a, out, host, pitch


class DevOnly:
    """A scalar argument that only the *_dev form has (a row pitch)."""
    def __init__(self, v):
        self.v = v


NULL = Arr(None)


def out(shape, dtype=np.uint8, pitch=None):
    return Arr(np.full(shape, FILL, np.uint8).repeat(np.dtype(dtype).itemsize, -1).view(dtype), out=True, pitch=pitch)


def _host_ptr(h):
    from flamingo_amd import _lib
    return {"uint32": _lib.p_u32, "float32": _lib.p_f32, "int64": _lib.p_i64, "int8": _lib.p_i8}.get(h.dtype.name, _lib.p_u8)(h)


def _run(eng, name, args, form, off8=None):
    """One call of `name` (host form) or `name`_dev on torch's stream.  args: the C arguments after ctx
    in order, arrays as Arr; off8: index into args of an array handed over 8 bytes off a 16-byte
    boundary (dev form).  -> (return code, flm_last_error, the output arrays' bytes after the call)."""
    import torch
    cargs, outs, alive = [], [], []                 # alive: the arrays, until the call has run
    for i, v in enumerate(args):
        if isinstance(v, DevOnly):
            if form == "dev":
                cargs.append(v.v)
            continue
        if not isinstance(v, Arr) or v.a is None:
            cargs.append(None if isinstance(v, Arr) else v)
            continue
        if form == "host" or v.host:
            h = np.ascontiguousarray(v.a).copy()
            cargs.append(_host_ptr(h))
            alive.append(h)
            fetch = h.tobytes
        else:
            a = np.ascontiguousarray(v.a)
            if v.pitch is not None:                  # rows `pitch` elements apart, the fill byte between them
                wide = np.full((a.shape[0], v.pitch * a.itemsize), FILL, np.uint8)
                wide[:, :a.shape[1] * a.itemsize] = a.view(np.uint8).reshape(a.shape[0], -1)
                a = wide
            raw = a.view(np.uint8).reshape(-1)
            shift = 8 if i == off8 else 0
            t = torch.zeros(raw.size + 16, dtype=torch.uint8, device="cuda")
            assert t.data_ptr() % 16 == 0
            t[shift:shift + raw.size] = torch.from_numpy(raw.copy())
            cargs.append(ctypes.c_void_p(t.data_ptr() + shift))
            alive.append(t)
            fetch = lambda t=t, shift=shift, n=raw.size: t[shift:shift + n].cpu().numpy().tobytes()  # noqa: E731
            if v.pitch is not None:                  # the rows' first words, as the host form returns them
                fetch = lambda f=fetch, r=v.a.shape[0], w=v.a.shape[1] * v.a.itemsize: np.frombuffer(  # noqa: E731
                    f(), np.uint8).reshape(r, -1)[:, :w].tobytes()
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


def _refused(eng, name, cases, misaligned=(), code=FLM_EINVAL):
    """each of `cases` (argument lists) is refused by both forms alike, outputs untouched; each
    (args, index) of `misaligned` by the *_dev form"""
    for args in cases:
        rc_h, err_h, got_h = _run(eng, name, args, "host")
        rc_d, err_d, got_d = _run(eng, name, args, "dev")
        assert rc_h == code and rc_d == code
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


# ================================================================== the round path
LS = (1, 5, 1025)
SEG = np.array([0, 0, 2, 3], np.int64)              # client 0 has no seeds; clients 1 and 2 have two and one
SIGNS = np.array([1, -1, -1], np.int8)


def _up4(L):
    return (L + 3) // 4 * 4


def _clients(N):
    """(seg, signs, seeds) of the first N clients of SEG: N = 1 is a client without seeds (K = 0)"""
    K = int(SEG[N])
    return Arr(SEG[:N + 1], host=True), Arr(SIGNS[:K], host=True) if K else Arr(np.zeros(1, np.int8), host=True), \
        Arr(_bytes(_rng(7, N), max(K, 1), 32))


@pytest.fixture
def small(eng):
    """sets the `small` tuning key for the test and puts it back"""
    before = eng.get_tuning("small")
    yield lambda v: eng.set_tuning("small", v)
    eng.set_tuning("small", before)


# ------------------------------------------------------------------ flm_client_mask
def _mask_args(N, L, with_x=True):
    seg, signs, seeds = _clients(N)
    x = Arr(_rng(8, N, L).integers(0, 1 << 32, (N, L), dtype=np.uint32), pitch=_up4(L)) if with_x else NULL
    return [x, DevOnly(_up4(L)), N, seg, seeds, signs, L, out((N, L), np.uint32, pitch=_up4(L))]


@pytest.mark.parametrize("L", LS)
@pytest.mark.parametrize("N", (1, 3))
@pytest.mark.parametrize("with_x", (True, False), ids=("x", "ones"))
def test_client_mask(eng, small, N, L, with_x):
    """the host form against the *_dev form's one-launch path (small = 2) and its work-item path (small = 0)"""
    args = _mask_args(N, L, with_x)
    small(2)
    one_launch = _same(eng, "flm_client_mask", args)
    small(0)
    assert _same(eng, "flm_client_mask", args) == one_launch
    if N == 1:                                       # no seeds: the input itself, or the all-ones row
        want = args[0].a if with_x else np.ones((1, L), np.uint32)
        assert one_launch[0] == want.tobytes()


def test_client_mask_refusals(eng):
    a = _mask_args(3, 5)
    bad = lambda v: Arr(np.array(v, np.int64), host=True)  # noqa: E731
    _refused(eng, "flm_client_mask", [_swap(a, 3, bad([1, 1, 2, 3])), _swap(a, 3, bad([0, 2, 1, 3])),
                                      _swap(a, 5, Arr(np.array([1, 0, 1], np.int8), host=True)), _swap(a, 3, NULL),
                                      _swap(a, 7, NULL), _swap(a, 4, NULL)],
             misaligned=[(a, 0), (a, 7)])
    for pitch in (4, 5):                             # below L; L itself, which is no multiple of 4
        rc, err, got = _run(eng, "flm_client_mask", _swap(a, 1, DevOnly(pitch)), "dev")
        assert rc == FLM_EINVAL and b"pitch" in err and set(got[0]) <= {FILL}


def test_client_mask_negative_n(eng):
    """the one documented difference: the host form refuses N = -1, the *_dev form returns 0; neither touches out"""
    a = _swap(_mask_args(3, 5), 2, -1)
    rc_h, err_h, got_h = _run(eng, "flm_client_mask", a, "host")
    rc_d, _, got_d = _run(eng, "flm_client_mask", a, "dev")
    assert rc_h == FLM_EINVAL and err_h and rc_d == 0
    assert set(got_h[0]) <= {FILL} and set(got_d[0]) <= {FILL}


def test_client_mask_dev_seeds_contiguous(eng):
    """MaskEngine reads seeds_dev 32 bytes apart: a strided view is refused by both client_*_dev wrappers"""
    import torch
    seeds = torch.zeros((3, 64), dtype=torch.uint8, device="cuda")[:, :32]
    o = torch.zeros((3, 8), dtype=torch.int32, device="cuda")
    with pytest.raises(RuntimeError, match="contiguous"):
        eng.client_mask_dev(SEG, seeds, SIGNS, o, 5)
    with pytest.raises(RuntimeError, match="contiguous"):
        eng.client_encode_mask_dev(SEG, seeds, SIGNS, o, 5, torch.zeros((3, 8), device="cuda"), 16, 4.0)


# ------------------------------------------------------------------ flm_client_encode_mask
F_BITS, CLIP = 16, 4.0


def _encode_args(N, L, dither=True, clipped=True, frac_bits=F_BITS, clip=CLIP):
    seg, signs, seeds = _clients(N)
    x = np.stack([C.random_row(L, CLIP, 100 * L + i, wild=True) for i in range(N)])
    if L < 4:
        x[0, 0] = 2 * CLIP                           # random_row sends nothing beyond the clip in so short a row
    d = Arr(_bytes(_rng(9, N), N, 32)) if dither else NULL
    return [Arr(x, pitch=_up4(L)), DevOnly(_up4(L)), N, seg, seeds, signs, L, frac_bits, clip, d,
            out((N, L), np.uint32, pitch=_up4(L)), DevOnly(_up4(L)), out((N,), np.uint32) if clipped else NULL]


@pytest.mark.parametrize("L", LS)
@pytest.mark.parametrize("N", (1, 3))
@pytest.mark.parametrize("opt", range(4), ids=("--", "d-", "-c", "dc"))
def test_client_encode_mask(eng, N, L, opt):
    got = _same(eng, "flm_client_encode_mask", _encode_args(N, L, bool(opt & 1), bool(opt & 2)))
    if opt & 2:
        assert np.frombuffer(got[1], np.uint32)[0] > 0   # some of client 0's values are clipped


def test_client_encode_mask_refusals(eng):
    a = _encode_args(3, 5)
    bad = lambda v: Arr(np.array(v, np.int64), host=True)  # noqa: E731
    _refused(eng, "flm_client_encode_mask",
             [_swap(a, 3, bad([1, 1, 2, 3])), _swap(a, 3, bad([0, 2, 1, 3])),
              _swap(a, 5, Arr(np.array([1, 0, 1], np.int8), host=True)), _swap(a, 3, NULL), _swap(a, 10, NULL),
              _swap(a, 0, NULL), _swap(a, 4, NULL), _swap(a, 7, 31), _swap(a, 8, 0.0), _swap(a, 8, float("inf")),
              _swap(a, 8, float("nan"))],
             misaligned=[(a, 0), (a, 10)])
    _refused(eng, "flm_client_encode_mask", [_swap(a, 8, 32768.5)], code=FLM_ERANGE)   # ceil(c 2^16) = 2^31 + 2^15
    for i in (1, 11):                                # x's pitch, out's
        for pitch in (4, 5):
            rc, err, got = _run(eng, "flm_client_encode_mask", _swap(a, i, DevOnly(pitch)), "dev")
            assert rc == FLM_EINVAL and b"pitch" in err and all(set(b) <= {FILL} for b in got)


# ------------------------------------------------------------------ flm_decode_sum
def _decode_args(L, frac_bits=F_BITS, count=3):
    words = np.resize(np.concatenate([C.DECODE_WORDS, _rng(10, L).integers(0, 1 << 32, L, dtype=np.uint32)]), L)
    return [Arr(words), L, frac_bits, count, out((L,), np.float32)]


@pytest.mark.parametrize("L", LS)
def test_decode_sum(eng, L):
    import torch
    a = _decode_args(L)
    got = _same(eng, "flm_decode_sum", a)
    assert got[0] == C.decode(a[0].a, F_BITS, 3).tobytes()
    t = torch.from_numpy(a[0].a.view(np.int32).copy()).cuda()      # out aliasing sum: decoded where it stands
    eng.decode_sum_dev(t, t.view(torch.float32), L, F_BITS, 3)
    assert t.cpu().numpy().tobytes() == got[0]


def test_decode_sum_refusals(eng):
    a = _decode_args(5)
    _refused(eng, "flm_decode_sum", [_swap(a, 2, 31), _swap(a, 3, 0), _swap(a, 0, NULL), _swap(a, 4, NULL)],
             misaligned=[(a, 0), (a, 4)])


# ------------------------------------------------------------------ flm_prg_expand
def _expand_args(K, L, slot0=0):
    return [Arr(_bytes(_rng(11, K), K, 32)), K, L, slot0, out((K, L), np.uint32, pitch=_up4(L)), DevOnly(_up4(L))]


@pytest.mark.parametrize("L", LS)
@pytest.mark.parametrize("K", (1, 3))
@pytest.mark.parametrize("slot0", (0, 16))
def test_prg_expand(eng, K, L, slot0):
    got = _same(eng, "flm_prg_expand", _expand_args(K, L, slot0))
    if slot0:                                        # the window 16 slots on is the first one's tail
        first = np.frombuffer(_run(eng, "flm_prg_expand", _expand_args(K, L + 16), "host")[2][0], np.uint32)
        assert got[0] == first.reshape(K, L + 16)[:, 16:].tobytes()


def test_prg_expand_refusals(eng):
    a = _expand_args(3, 5)
    _refused(eng, "flm_prg_expand", [_swap(a, 3, 8), _swap(a, 0, NULL), _swap(a, 4, NULL)], misaligned=[(a, 4)])
    _refused(eng, "flm_prg_expand", [_swap(_expand_args(1, 1), 3, 1 << 36)], code=FLM_ERANGE)  # before any allocation
    for pitch in (4, 5):
        rc, err, got = _run(eng, "flm_prg_expand", _swap(a, 5, DevOnly(pitch)), "dev")
        assert rc == FLM_EINVAL and b"pitch" in err and set(got[0]) <= {FILL}


# ------------------------------------------------------------------ flm_mask_accumulate, flm_aggregate_unmask
def _round_dev(eng, rows, seeds, signs, L, slot0=0):
    """flm_aggregate_unmask_dev on MaskEngine's device arrays: rows (N, L) at a pitch of round_up(L, 4)"""
    import torch
    N, K = rows.shape[0], len(signs)
    d_rows = torch.zeros((max(N, 1), _up4(L)), dtype=torch.int32, device="cuda")
    d_rows[:N, :L] = torch.from_numpy(rows.view(np.int32))
    d_out = torch.full((_up4(L),), FILL * 0x01010101, dtype=torch.int32, device="cuda")
    eng.aggregate_unmask_dev(d_rows[:N], torch.from_numpy(seeds[:K]).cuda() if K else None,
                             torch.from_numpy(signs[:K]).cuda() if K else None, d_out, L=L, prg_slot0=slot0)
    torch.cuda.synchronize()
    return d_out.cpu().numpy().view(np.uint32)[:L]


@pytest.mark.parametrize("L", LS)
@pytest.mark.parametrize("K", (0, 3))
def test_mask_accumulate(eng, K, L):
    from flamingo_amd._lib import p_i8, p_u8, p_u32
    seeds, acc = _bytes(_rng(12, K), 3, 32), _rng(13, L).integers(0, 1 << 32, (1, L), dtype=np.uint32)
    for slot0 in (0, 16):
        h = acc.copy()
        assert eng.lib.flm_mask_accumulate(eng.ctx, p_u8(seeds), p_i8(SIGNS), K, p_u32(h), L, slot0) == 0
        assert (h[0] == _round_dev(eng, acc, seeds, SIGNS[:K], L, slot0)).all()
        assert K == 0 or (h != acc).any()


@pytest.mark.parametrize("L", LS)
@pytest.mark.parametrize("N,K", ((0, 3), (3, 0), (3, 3)))
def test_aggregate_unmask(eng, N, K, L):
    seeds, rows = _bytes(_rng(14, K), 3, 32), _rng(15, N, L).integers(0, 1 << 32, (N, L), dtype=np.uint32)
    got = eng.aggregate_unmask(list(rows), seeds[:K], SIGNS[:K], L=L)
    assert (got == _round_dev(eng, rows, seeds, SIGNS[:K], L)).all()
    if K == 0:
        assert (got == rows.sum(0, dtype=np.uint32)).all()


def test_round_refusals(eng):
    """a sign of 0, NULL seeds with K > 0 and a NULL out: the host calls and flm_aggregate_unmask_dev alike"""
    import torch
    from flamingo_amd._lib import p_i8, p_u8, p_u32
    lib, ctx, L = eng.lib, eng.ctx, 5
    seeds, zero = _bytes(_rng(16), 3, 32), np.array([1, 0, 1], np.int8)
    acc = np.full(L, FILL * 0x01010101, np.uint32)
    d_acc = torch.from_numpy(np.resize(acc, 8).view(np.int32)).cuda()
    d_seeds, d_signs = torch.from_numpy(seeds).cuda(), torch.from_numpy(SIGNS).cuda()
    dev = lambda sd, sg, o: lib.flm_aggregate_unmask_dev(  # noqa: E731
        ctx, d_acc.data_ptr(), 8, 1, sd, sg, 3, L, 0, L, 0, o, eng._stream_handle(None))
    texts = []
    for rc in (lib.flm_mask_accumulate(ctx, None, p_i8(SIGNS), 3, p_u32(acc), L, 0),
               lib.flm_aggregate_unmask(ctx, None, 0, None, p_i8(SIGNS), 3, L, p_u32(acc)),
               dev(None, d_signs.data_ptr(), d_acc.data_ptr())):
        assert rc == FLM_EINVAL
        texts.append(lib.flm_last_error(ctx))
    assert len(set(texts)) == 1 and texts[0]
    texts = []
    for rc in (lib.flm_mask_accumulate(ctx, p_u8(seeds), p_i8(SIGNS), 3, None, L, 0),
               lib.flm_aggregate_unmask(ctx, None, 0, p_u8(seeds), p_i8(SIGNS), 3, L, None),
               dev(d_seeds.data_ptr(), d_signs.data_ptr(), None)):
        assert rc == FLM_EINVAL
        texts.append(lib.flm_last_error(ctx))
    assert len(set(texts)) == 1 and texts[0]
    assert lib.flm_mask_accumulate(ctx, p_u8(seeds), p_i8(zero), 3, p_u32(acc), L, 0) == FLM_EINVAL
    sign_text = lib.flm_last_error(ctx)
    assert lib.flm_aggregate_unmask(ctx, None, 0, p_u8(seeds), p_i8(zero), 3, L, p_u32(acc)) == FLM_EINVAL
    assert lib.flm_last_error(ctx) == sign_text and b"signs" in sign_text
    assert lib.flm_mask_accumulate(ctx, p_u8(seeds), p_i8(SIGNS), 3, p_u32(acc), L, 8) == FLM_EINVAL
    assert lib.flm_mask_accumulate(ctx, p_u8(seeds), p_i8(SIGNS), 3, p_u32(acc), 1, 1 << 36) == FLM_ERANGE
    torch.cuda.synchronize()
    assert set(acc.tobytes()) == {FILL} and set(d_acc.cpu().numpy().tobytes()) == {FILL}
