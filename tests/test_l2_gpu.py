"""The L2 clip's kernels bit for bit against the numpy restatement (tests/l2_cases.py): the sums of squares and the
factors at rows around the 16-parameter thread, the 4096-parameter tile and the 64-partial row sum, with NaN in every
row's padding; the factor's edges and the order-sensitive rows; the square-root pins; the scale pass with guards; the
fused forward rotation against the restatement, against the two-pass device path and beside the unchanged rotation; the
host forms, the reference-side binding and the stream contract.  NaN compares as NaN, everything else by its bits."""
from __future__ import annotations

import ctypes
import importlib.util
import os

import numpy as np
import pytest

import l2_cases as l2
import rotate_cases as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = np.float32(-123456.75)
FLM_EINVAL = -1   # include/flamingo_hip.h


@pytest.fixture(scope="module")
def eng():
    from flamingo_amd import MaskEngine
    e = MaskEngine(0)
    yield e
    e.close()


def _same(got, want):
    return np.array_equal(R.bits(got), R.bits(want))


def _signs(L_rot, key=R.KEY):
    import torch
    return torch.from_numpy(R.sign_words(key, L_rot).view(np.int32).copy()).cuda()


def _padded(xs, pitch, fill=np.nan):
    """the rows at `pitch` floats, `fill` behind each"""
    import torch
    buf = np.full((xs.shape[0], pitch), fill, np.float32)
    buf[:, :xs.shape[1]] = xs
    return torch.from_numpy(buf).cuda()


def _factors(eng, t, L, C):
    """flm_l2_factors_dev on the device rows t: (factors, sumsq) as numpy, from buffers that held other values."""
    import torch
    N = t.shape[0]
    work = torch.full((eng.l2_clip_check(L, C, N),), float("nan"), dtype=torch.float64, device="cuda")
    f = torch.full((N,), 77.0, dtype=torch.float32, device="cuda")
    S = torch.full((N,), -1.0, dtype=torch.float64, device="cuda")
    eng.l2_factors_dev(t, L, C, work, f, S)
    return f, S.cpu().numpy()


def _want(xs, C):
    r = [l2.clip(x, C) for x in xs]
    return np.stack([y for y, _, _ in r]), np.array([s for _, s, _ in r], np.float32), np.array([S for _, _, S in r], np.float64)


# ------------------------------------------------------------------ sums of squares and factors
@pytest.mark.parametrize("L", l2.LENGTHS)
def test_factors_match_the_restatement(eng, L):
    C = 1.0
    for N in (1, 3):
        xs = l2.rows(N, L, 300 + N + L % 97, C)
        _, fw, Sw = _want(xs, C)
        assert fw[0] == 1.0 and (N == 1 or fw[1] < 1.0)                       # rows inside and outside the norm
        f, S = _factors(eng, _padded(xs, (L + 3) // 4 * 4 + 16), L, C)        # pitch > L, NaN behind every row
        assert S.tobytes() == Sw.tobytes(), (L, N)
        assert f.cpu().numpy().tobytes() == fw.tobytes(), (L, N)
    # the last row alone, at another pitch, with other values behind it: the same bits
    f1, S1 = _factors(eng, _padded(xs[2:], (L + 3) // 4 * 4 + 64, 1e30), L, C)
    assert S1.tobytes() == Sw[2:].tobytes() and f1.cpu().numpy().tobytes() == fw[2:].tobytes()
    # sumsq is optional
    import torch
    work = torch.empty(eng.l2_clip_check(L, C, 3), dtype=torch.float64, device="cuda")
    f = torch.zeros(3, dtype=torch.float32, device="cuda")
    eng.l2_factors_dev(_padded(xs, (L + 3) // 4 * 4), L, C, work, f)
    assert f.cpu().numpy().tobytes() == fw.tobytes()


def test_factor_edges_and_order_sensitive_rows(eng):
    L = l2.SPECIAL_L
    for C, xs, names in l2.special_batches():
        yw, fw, Sw = _want(xs, C)
        t = _padded(xs, L + 3 + 8)
        f, S = _factors(eng, t, L, C)
        for i, name in enumerate(names):
            assert S[i].tobytes() == Sw[i].tobytes(), (C, name, S[i], Sw[i])
            assert f.cpu().numpy()[i].tobytes() == fw[i].tobytes(), (C, name)
        got, hf, hS = eng.l2_clip(xs, C)                                        # the host form: factors, then the scale
        assert _same(got, yw) and hf.tobytes() == fw.tobytes() and hS.tobytes() == Sw.tobytes(), C
    order = l2.order_rows()
    S = _factors(eng, _padded(order, L + 3), L, 5.0)[1]
    assert all(S[i].tobytes() != l2.sequential_sumsq(x).tobytes() for i, x in enumerate(order))


def test_square_root_pins(eng):
    """S = n 4^e by construction (sumsq must return it exactly) and factors = float32(C / sqrt(S)) with C = 2^e.  The
    factor is a float32: it shows a wrong last bit of the double root only where that moves C / sqrt(S) across a
    float32 rounding boundary, so this pins the perfect squares and the magnitude, not every last bit."""
    pins = l2.sqrt_pins()
    for e in sorted({e for _, e in pins}):
        C = float(np.ldexp(1.0, e))
        group = [n for n, ee in pins if ee == e]
        xs = np.stack([l2.row_with_sumsq(n, e, 64) for n in group])
        f, S = _factors(eng, _padded(xs, 64 + 4), 64, C)
        f = f.cpu().numpy()
        for i, n in enumerate(group):
            want = l2.double_of(n, e)
            assert S[i].tobytes() == want.tobytes(), (n, e)
            assert f[i].tobytes() == l2.factor(want, C).tobytes() and f[i] < 1.0, (n, e)
    # perfect squares: the root is exact, so C / y is one division
    for y in (3, 5, 2 ** 24 - 1, 94906265):
        f, S = _factors(eng, _padded(l2.row_with_sumsq(y * y, 0, 64)[None, :], 64), 64, 1.0)
        assert S[0] == float(y * y) and f.cpu().numpy()[0] == np.float32(1.0 / y)


# ------------------------------------------------------------------ the scale pass
@pytest.mark.parametrize("L", (1, 17, 4097, 8193))
def test_scale_rows_in_place_and_out_of_place(eng, L):
    import torch
    xs = R.rows(4, L, 500 + L)
    xs[0, 0], xs[1, L - 1], xs[2, L // 2], xs[3, 0] = -0.0, 1e-45, np.nan, -np.inf
    xs[1, 0] = -3e-42
    fs = np.array([0.3, 1.0, 4.5956e-41, 0.5], np.float32)                      # a subnormal factor among them
    with np.errstate(invalid="ignore", under="ignore"):
        want = (xs * fs[:, None]).astype(np.float32)
    assert want[1].tobytes() == xs[1].tobytes()
    factors = torch.from_numpy(fs).cuda()
    XP, OP = (L + 3) // 4 * 4 + 16, (L + 3) // 4 * 4 + 32
    out = torch.full((4, OP), float(GUARD), dtype=torch.float32, device="cuda")
    eng.scale_rows_dev(_padded(xs, XP), out, L, factors)
    got = out.cpu().numpy()
    assert _same(got[:, :L], want) and np.all(got[:, L:].view(np.uint32) == GUARD.view(np.uint32))
    assert got[1, :L].tobytes() == xs[1].tobytes()                              # a factor of 1 keeps every bit
    t = _padded(xs, XP, float(GUARD))
    eng.scale_rows_dev(t, t, L, factors)
    got = t.cpu().numpy()
    assert _same(got[:, :L], want) and np.all(got[:, L:].view(np.uint32) == GUARD.view(np.uint32))
    rc = eng.lib.flm_scale_rows_dev(eng.ctx, t.data_ptr(), XP, 2, L, factors.data_ptr(), t.data_ptr(), XP + 4,
                                    eng._stream_handle(None))
    with pytest.raises(RuntimeError, match="equal pitches"):                    # in place needs them
        eng._check(rc, "flm_scale_rows_dev")


# ------------------------------------------------------------------ the fused forward rotation
@pytest.mark.parametrize("h", (4, 5, 8, 9, 12))
def test_rotate_clip_matches_the_restatement_and_the_two_pass_path(eng, h):
    import torch
    C, N = 1.0, 3
    L = 2 * 4096 + (1 << h) // 2 + 3
    L_rot = R.rotated_len(L, h)
    assert eng.rotate_check(L, h) == L_rot
    xs = l2.rows(N, L, 700 + h, C)
    xs[1, 0], xs[1, 4095], xs[1, L - 1], xs[2, 4096] = np.nan, np.inf, -np.inf, np.nan
    want = [l2.clip_forward(x, C, R.KEY, h) for x in xs]
    yw = np.stack([w[0] for w in want])
    assert [w[1] for w in want] == [0, 3, 1] and want[0][2] == 1.0 and want[1][2] < 1.0
    sb = _signs(L_rot)
    x = _padded(xs, (L + 3) // 4 * 4 + 16)
    f, S = _factors(eng, x, L, C)
    assert S.tobytes() == np.array([w[3] for w in want]).tobytes()              # non-finite inputs are absent from S
    assert f.cpu().numpy().tobytes() == np.array([w[2] for w in want], np.float32).tobytes()
    out = torch.full((N, L_rot + 32), float(GUARD), dtype=torch.float32, device="cuda")
    cnt = torch.full((N,), 77, dtype=torch.int32, device="cuda")
    eng.rotate_clip_dev(x, out, L, h, sb, f, nonfinite=cnt)
    got = out.cpu().numpy()
    assert _same(got[:, :L_rot], yw) and np.all(got[:, L_rot:].view(np.uint32) == GUARD.view(np.uint32))
    assert list(cnt.cpu().numpy()) == [0, 3, 1]
    # flm_scale_rows_dev, then flm_rotate_dev: the same bits and counts
    mid = torch.empty((N, (L + 3) // 4 * 4), dtype=torch.float32, device="cuda")
    two = torch.empty((N, L_rot), dtype=torch.float32, device="cuda")
    cnt2 = torch.zeros((N,), dtype=torch.int32, device="cuda")
    eng.scale_rows_dev(x, mid, L, f)
    eng.rotate_dev(mid, two, L, h, sb, nonfinite=cnt2)
    assert two.cpu().numpy().tobytes() == got[:, :L_rot].tobytes() and list(cnt2.cpu().numpy()) == [0, 3, 1]
    # in place at equal pitches
    t = _padded(xs, L_rot + 8)
    eng.rotate_clip_dev(t, t, L, h, sb, f)
    again = t.cpu().numpy()
    assert _same(again[:, :L_rot], yw) and np.isnan(again[:, L_rot:]).all()
    # the rotation alone, in the same process on the same inputs: what it always gave
    plain = torch.empty((N, L_rot), dtype=torch.float32, device="cuda")
    eng.rotate_dev(x, plain, L, h, sb, nonfinite=cnt2)
    assert _same(plain.cpu().numpy(), np.stack([R.forward(r, R.KEY, h)[0] for r in xs]))
    assert list(cnt2.cpu().numpy()) == [0, 3, 1]


# ------------------------------------------------------------------ host forms, the binding, the stream
@pytest.mark.parametrize("N", (1, 3))
def test_host_forms_equal_device_forms(eng, N, monkeypatch):
    import torch
    h, L, C = 9, 4096 + 700, 0.75
    L_rot = R.rotated_len(L, h)
    xs = l2.rows(N, L, 80 + N, C)
    xs[0, 5] = np.inf
    x = torch.from_numpy(xs).cuda()
    f, S = _factors(eng, x, L, C)
    scaled = torch.empty((N, L), dtype=torch.float32, device="cuda")
    eng.scale_rows_dev(x, scaled, L, f)
    rot = torch.empty((N, L_rot), dtype=torch.float32, device="cuda")
    cnt = torch.zeros((N,), dtype=torch.int32, device="cuda")
    eng.rotate_clip_dev(x, rot, L, h, _signs(L_rot), f, nonfinite=cnt)
    out, hf, hS = eng.l2_clip(xs, C)
    assert _same(out, scaled.cpu().numpy()) and hf.tobytes() == f.cpu().numpy().tobytes() and hS.tobytes() == S.tobytes()
    y, bad, rf, rS = eng.rotate(xs, R.KEY, h, return_nonfinite=True, clip_norm=C)
    assert y.shape == (N, L_rot) and y.tobytes() == rot.cpu().numpy().tobytes()
    assert list(bad) == list(cnt.cpu().numpy()) and bad[0] == 1 and rf.tobytes() == hf.tobytes() and rS.tobytes() == hS.tobytes()
    y2, rf2, rS2 = eng.rotate(xs, R.KEY, h, clip_norm=C)
    assert y2.tobytes() == y.tobytes() and rf2.tobytes() == rf.tobytes()
    want = [l2.clip_forward(r, C, R.KEY, h) for r in xs]
    assert _same(y, np.stack([w[0] for w in want])) and rS.tobytes() == np.array([w[3] for w in want]).tobytes()
    # without clip_norm: today's call and today's result
    plain, bad0 = eng.rotate(xs, R.KEY, h, return_nonfinite=True)
    assert _same(plain, np.stack([R.forward(r, R.KEY, h)[0] for r in xs])) and list(bad0) == list(bad)
    assert eng.rotate(xs, R.KEY, h).tobytes() == plain.tobytes()
    if N == 1:
        # a vector in, a vector out; and the reference-side binding, call for call
        v, vf, vS = eng.l2_clip(xs[0], C)
        assert v.shape == (L,) and v.tobytes() == out[0].tobytes() and vS.tobytes() == hS.tobytes()
        monkeypatch.setenv("FLM_LIB", os.path.join(ROOT, "flamingo_amd", "lib", "libflamingo_hip.so"))
        spec = importlib.util.spec_from_file_location("util_flm", os.path.join(ROOT, "integration", "util_flm.py"))
        flm = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(flm)
        assert flm.l2_clip_check(L, C) == eng.l2_clip_check(L, C) == 2 and flm.l2_clip_check(L, C, 3) == 6
        with pytest.raises(RuntimeError):
            flm.l2_clip_check(L, 0.0)
        u, us, uS = flm.l2_clip(xs[0], C)
        assert u.tobytes() == out[0].tobytes() and np.float32(us) == hf[0] and uS == hS[0]
        r, rb, rs, rS1 = flm.rotate(xs[0], R.KEY, h, clip_norm=C)
        assert r.tobytes() == y[0].tobytes() and rb == 1 and np.float32(rs) == rf[0] and rS1 == rS[0]
        p, pb = flm.rotate(xs[0], R.KEY, h)
        assert p.tobytes() == plain[0].tobytes() and pb == 1
        assert flm.rotate(p, R.KEY, h, inverse=True, L=L).tobytes() == eng.rotate(plain, R.KEY, h, inverse=True, L=L)[0].tobytes()


def test_refusals_on_the_device(eng):
    import torch
    L = 100
    x = torch.zeros((2, 104), dtype=torch.float32, device="cuda")
    work = torch.zeros(2, dtype=torch.float64, device="cuda")
    f = torch.ones(2, dtype=torch.float32, device="cuda")
    for C in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(RuntimeError):
            eng.l2_factors_dev(x, L, C, work, f)
    with pytest.raises(RuntimeError):
        eng.l2_factors_dev(x, L, 1.0, work[:1], f)                              # too little work space
    with pytest.raises(RuntimeError):
        eng.l2_factors_dev(x[:, 1:], L, 1.0, work, f)                           # rows off 16 bytes
    with pytest.raises(RuntimeError):
        eng.l2_clip(np.zeros((2, 5), np.float32), 0.0)
    with pytest.raises(RuntimeError):
        eng.rotate(np.zeros((2, 32), np.float32), R.KEY, 5, inverse=True, L=20, clip_norm=1.0)
    # The C calls themselves, where flm_rotate_clip[_dev] differ from flm_rotate[_dev] (tests/test_rotate_gpu.py has
    # those): every case returns before a launch, so one-element tensors and NULL stand in for the arrays.
    lib, ctx, stream, h = eng.lib, eng.ctx, eng._stream_handle(None), 5
    one = torch.zeros(4, dtype=torch.float32, device="cuda")
    p = ctypes.c_void_p(one.data_ptr())

    def refused(rc, text):
        return rc == FLM_EINVAL and text in lib.flm_last_error(ctx)

    # the host form asks the L2 rule, which wants a row: N = 0 is no early return there
    for N in (-1, 0):
        assert refused(lib.flm_rotate_clip(ctx, None, N, L, h, None, 1.0, None, None, None, None), b"N must be at least 1")
    # ... after the rotation's own rule: a bad block and a bad radius give the block's message
    assert refused(lib.flm_rotate_clip(ctx, None, 1, L, 3, None, 0.0, None, None, None, None), b"log2_block outside 4..12")
    assert refused(lib.flm_rotate_clip(ctx, None, 1, L, h, None, 0.0, None, None, None, None), b"clip_norm must be finite")
    # the device form takes its factors from elsewhere and asks no L2 rule: N = 0 is nothing to do, N < 0 the rotation's
    assert lib.flm_rotate_clip_dev(ctx, None, 0, 0, L, h, None, None, None, 0, None, stream) == 0
    assert refused(lib.flm_rotate_clip_dev(ctx, None, 0, -1, L, h, None, None, None, 0, None, stream), b"negative N")
    # ... and its factors are an array like the rows: NULL is refused, behind the rotation's rule
    assert refused(lib.flm_rotate_clip_dev(ctx, p, 104, 1, L, h, p, None, p, 128, None, stream), b"NULL argument")
    assert refused(lib.flm_rotate_clip_dev(ctx, p, 104, 1, L, 3, p, None, p, 128, None, stream), b"log2_block outside 4..12")


def test_dev_call_returns_before_its_stream_drains(eng):
    """The stream contract (tests/test_streams_gpu.py): queued behind a chain of large matmuls, each call returns
    while that chain still runs, and the results read afterwards in stream order are right."""
    import torch
    C, L, N, h = 1.0, 4096 + 11, 3, 8
    L_rot = R.rotated_len(L, h)
    xs = l2.rows(N, L, 90, C)
    x, sb = torch.from_numpy(np.ascontiguousarray(np.pad(xs, ((0, 0), (0, 1))))).cuda(), _signs(L_rot)
    work = torch.empty(eng.l2_clip_check(L, C, N), dtype=torch.float64, device="cuda")
    f = torch.zeros(N, dtype=torch.float32, device="cuda")
    S = torch.zeros(N, dtype=torch.float64, device="cuda")
    out = torch.empty((N, L_rot), dtype=torch.float32, device="cuda")
    scaled = torch.empty((N, L + 1), dtype=torch.float32, device="cuda")
    eng.l2_factors_dev(x, L, C, work, f, S)                                     # warm
    torch.cuda.synchronize()
    a = torch.ones((8192, 8192), device="cuda")
    for _ in range(12):
        a = a @ a * 1e-4
    busy = torch.cuda.Event()
    busy.record()
    eng.l2_factors_dev(x, L, C, work, f, S)
    eng.scale_rows_dev(x, scaled, L, f)
    eng.rotate_clip_dev(x, out, L, h, sb, f)
    assert not busy.query(), "an L2 clip _dev call waited for earlier work on its stream"
    torch.cuda.synchronize()
    want = [l2.clip_forward(r, C, R.KEY, h) for r in xs]
    assert _same(out.cpu().numpy(), np.stack([w[0] for w in want]))
    assert _same(scaled.cpu().numpy()[:, :L], np.stack([l2.clip(r, C)[0] for r in xs]))
    assert S.cpu().numpy().tobytes() == np.array([w[3] for w in want]).tobytes()
