"""The L2 clip without a GPU: the premises of tests/l2_cases.py (the restatement the kernels are held to bit for bit by
tests/test_l2_gpu.py), the library's rule and refusals, and the agents' options."""
from __future__ import annotations

import ctypes
import math

import numpy as np
import pytest

import l2_cases as l2
import pack_cases as PC
import rotate_cases as R

FLM_EINVAL, FLM_ERANGE = -1, -4     # include/flamingo_hip.h


@pytest.fixture(scope="module")
def lib():
    from flamingo_amd import build, _lib
    build.build()
    return _lib.load()


def _exact_norm(x) -> float:
    return math.sqrt(math.fsum(float(v) * float(v) for v in np.asarray(x, np.float32)))


# ------------------------------------------------------------------ the restatement
def test_sum_is_within_its_bound_of_the_exact_sum():
    for L in l2.LENGTHS:
        for x in l2.rows(2, L, 40 + L % 89, 1.0):
            S, exact = float(l2.sumsq(x)), math.fsum(float(v) for v in l2.squares(x))
            assert abs(S - exact) <= L * 2.0 ** -53 * exact, L
    # a row of one tile is one partial; padding and non-finite elements count as +0.0
    x = l2.rows(1, 100, 3, 1.0)[0]
    assert l2.sumsq(x) == l2.tile_partials(x)[0] and len(l2.tile_partials(np.ones(4097, np.float32))) == 2
    y = np.concatenate([x, [np.nan, np.inf, -np.inf]]).astype(np.float32)
    assert l2.sumsq(y) == l2.sumsq(x) == l2.sumsq(np.concatenate([x, np.zeros(5000, np.float32)]))
    assert l2.sumsq(np.full(7, np.nan, np.float32)).tobytes() == np.float64(0.0).tobytes()


def test_the_order_rows_tell_the_normative_order_from_a_sequential_sum():
    rows = l2.order_rows()
    assert len(rows) >= 3
    for x in rows:
        S, seq, exact = l2.sumsq(x), l2.sequential_sumsq(x), math.fsum(float(v) for v in l2.squares(x))
        assert S.tobytes() != seq.tobytes()
        assert abs(float(S) - exact) <= len(x) * 2.0 ** -53 * exact
        assert abs(float(S) - exact) < abs(float(seq) - exact)     # the sequential sum lost the ones behind 1e16


def test_rows_with_a_chosen_sum():
    for n, e in [(25 << 48, -24), ((25 << 48) + 1, -24), ((25 << 48) - 1, -24), (2 ** 53 - 1, 0), (1, -60), (7, 3)]:
        x = l2.row_with_sumsq(n, e)
        want = l2.double_of(n, e)
        assert float(want) == math.ldexp(n, 2 * e) and l2.sumsq(x) == want and l2.sequential_sumsq(x) == want
        assert l2.sumsq(x[::-1].copy()) == want and l2.sumsq(l2.row_with_sumsq(n, e, 5000)) == want


def test_factor_edges():
    one = np.float32(1.0)
    assert l2.factor(0.0, 5.0) == one and l2.factor(25.0, 5.0) == one
    assert l2.factor(np.nextafter(25.0, 0.0), 5.0) == one
    above = np.nextafter(np.float64(25.0), np.inf)
    assert l2.factor(above, 5.0) == np.float32(5.0 / np.sqrt(above)) <= one
    assert l2.factor(100.0, 5.0) == np.float32(0.5) and l2.factor(1e-90, 1e-40) == one
    # C is taken as a float32, and C^2 is exact in float64
    c = np.float32(0.3)
    assert l2.factor(np.float64(c) * np.float64(c), 0.3) == one
    assert l2.factor(np.nextafter(np.float64(c) * np.float64(c), np.inf), 0.3) <= one
    for C, rows, names in l2.special_batches():
        for x, name in zip(rows, names):
            y, s, S = l2.clip(x, C)
            assert s.dtype == np.float32 and 0.0 < s <= 1.0, name
            if name in ("zero", "3-4-5", "25 exactly", "one ulp below", "tiny within") or "least" in name:
                assert s == one and y.tobytes() == x.tobytes(), name          # -0.0 and subnormals keep their bits
            if name == "zero":
                assert S.tobytes() == np.float64(0.0).tobytes()
            if name in ("3-4-5", "25 exactly"):
                assert S == 25.0
            if name == "one ulp above":
                assert S == above
            if name == "one ulp below":
                assert S == np.nextafter(np.float64(25.0), 0.0)
            if "3.4e38" in name or "alternating" in name:                       # S about 4.7e80, a subnormal factor
                assert 4.7e80 < S < 4.8e80 and 0.0 < s < np.finfo(np.float32).tiny and np.all(np.isfinite(y))
            if "outside" in name or name.startswith("order"):
                assert s < one, name
    tiny = l2.special_batches()[0][1][5]
    assert np.signbit(tiny[3]) and tiny[3] == 0.0 and 0.0 < tiny[0] < np.finfo(np.float32).tiny


def test_clipped_rows_stay_within_the_documented_bound():
    rng = np.random.default_rng(1)
    worst = 0.0
    for L in (1, 15, 16, 17, 4095, 4096, 4097, 8193, 100003):
        for C in (1.0, 0.3, 7.5, 1e-3):
            for scale in (1e-3, 1.0, 50.0, 1e10, 1e-20):
                x = (rng.standard_normal(L) * scale).astype(np.float32)
                y, s, S = l2.clip(x, C)
                norm, Cf = _exact_norm(y), float(np.float32(C))
                worst = max(worst, norm / Cf - 1.0)
                assert norm <= Cf * l2.BOUND, (L, C, scale)
                if s == 1.0:
                    assert y.tobytes() == x.tobytes()
                else:
                    assert norm >= Cf * (1.0 - 2.0 ** -22), (L, C, scale)  # scaled onto the sphere, not inside it
    assert worst < 2.0 ** -23
    for C, rows, names in l2.special_batches()[:2]:              # the order rows and the rows of 3.4e38 too
        for x, name in zip(rows, names):
            y = l2.clip(x, C)[0]
            if np.all((y == 0) | (np.abs(y) >= np.finfo(np.float32).tiny)):
                assert _exact_norm(y) <= float(np.float32(C)) * l2.BOUND, name


def test_clip_composes_with_the_rotation():
    x = l2.rows(2, 300, 9, 1.0)[1]
    x[[0, 17, 299]] = np.nan, np.inf, -np.inf
    y, bad, s, S = l2.clip_forward(x, 1.0, R.KEY, 6)
    assert bad == 3 and s < 1.0 and len(y) == 320
    # the multiply between the zeroing and the flips: the same bits, because a flip commutes with a multiply
    clean = np.where(np.isfinite(x), x, np.float32(0.0)).astype(np.float32)
    v = np.zeros(320, np.float32)
    v[:300] = R._flip(clean, R.sign_mask(R.KEY, 320)[:300]) * s
    v[:300] = np.where(np.isfinite(x), v[:300], R._flip(np.zeros(300, np.float32), R.sign_mask(R.KEY, 320)[:300]))
    v[300:] = R._flip(np.zeros(20, np.float32), R.sign_mask(R.KEY, 320)[300:])
    assert np.array_equal(R.bits(R._stages(v, 6)), R.bits(y))
    assert S == l2.sumsq(clean)


def test_one_hot_of_height_100_never_reaches_the_coordinate_clip():
    c = R.ONE_HOT
    x = np.zeros(c["L"], np.float32)
    x[70] = 100.0
    y, bad, s, S = l2.clip_forward(x, c["c"], R.KEY, c["h"])
    assert S == 1e4 and bad == 0
    blk = y[64:128]
    assert np.all(np.abs(blk) == 2.0 ** -5) and not y[:64].any()
    assert int(PC.encode_packed(y, c["f"], c["c"], c["pack"])[1].sum()) == 0        # clip >= C never fires
    plain = R.forward(x, R.KEY, c["h"])[0]
    assert np.all(np.abs(plain[64:128]) == 12.5)
    assert int(PC.encode_packed(plain, c["f"], c["c"], c["pack"])[1].sum()) == 64   # without the L2 clip it does


def test_square_root_pins_are_what_they_claim():
    pins = l2.sqrt_pins()
    assert len(pins) >= 40
    near = 0
    for n, e in pins:
        S = l2.double_of(n, e)
        x = l2.row_with_sumsq(n, e)
        assert l2.sumsq(x) == S
        y = float(np.sqrt(S))
        m, ex = math.frexp(y)
        Y = int(m * 2 ** 53)                                      # y = Y 2^(ex - 53)
        sh = 2 * (ex - 53) - 2 * e                                # y^2 = Y^2 2^sh in units of 4^e
        lo, hi = (2 * Y - 1) ** 2, (2 * Y + 1) ** 2               # (2 (y -+ ulp / 2))^2 = these 2^sh
        t = 4 * n
        if sh >= 0:
            lo, hi = lo << sh, hi << sh
        else:
            t <<= -sh
        assert lo <= t <= hi, (n, e)                              # numpy's root is the correctly rounded one
        near += min(t - lo, hi - t) * 2 ** 90 < t
    assert near >= 12                                             # ... and some roots are within 2^-90 of half-way


# ------------------------------------------------------------------ the library, no device
def test_l2_clip_check_values_and_refusals(lib):
    out = ctypes.c_uint64(0)
    for L in l2.LENGTHS + (4001, 1 << 20):
        for N in (1, 3, 1024):
            assert lib.flm_l2_clip_check(L, 1.0, N, ctypes.byref(out)) == 0 and out.value == N * -(-L // 4096), (L, N)
    assert lib.flm_l2_clip_check(100, 0.5, 1, None) == 0
    assert lib.flm_l2_clip_check(0, 1.0, 1, ctypes.byref(out)) == FLM_EINVAL
    for N in (0, -1):
        assert lib.flm_l2_clip_check(100, 1.0, N, ctypes.byref(out)) == FLM_EINVAL
    for C in (0.0, -1.0, float("inf"), float("nan"), -0.0):
        assert lib.flm_l2_clip_check(100, C, 1, ctypes.byref(out)) == FLM_EINVAL, C
    assert b"clip_norm" in lib.flm_last_error(None)
    assert lib.flm_l2_clip_check(100, 1e-45, 1, ctypes.byref(out)) == 0          # the least subnormal is positive
    # N ceil(L / 4096) <= 2^31 - 1 workgroups
    assert lib.flm_l2_clip_check(4096 * (2 ** 31 - 1), 1.0, 1, ctypes.byref(out)) == 0 and out.value == 2 ** 31 - 1
    assert lib.flm_l2_clip_check(4096 * (2 ** 31 - 1) + 1, 1.0, 1, ctypes.byref(out)) == FLM_ERANGE
    assert b"2^31" in lib.flm_last_error(None)
    assert lib.flm_l2_clip_check(4096 * 2 ** 20, 1.0, 2048, ctypes.byref(out)) == FLM_ERANGE
    assert lib.flm_l2_clip_check(2 ** 64 - 1, 1.0, 1, ctypes.byref(out)) == FLM_ERANGE
    assert lib.flm_l2_clip_check(2 ** 64 - 1, 1.0, 0, ctypes.byref(out)) == FLM_EINVAL


def test_l2_calls_reject_null_handles(lib):
    x = (ctypes.c_float * 16)()
    key = (ctypes.c_uint8 * 32)()
    cnt = (ctypes.c_uint32 * 1)()
    s = (ctypes.c_float * 1)()
    S = (ctypes.c_double * 1)()
    assert lib.flm_l2_clip(None, x, 1, 16, 1.0, x, s, S) == FLM_EINVAL
    assert b"NULL" in lib.flm_last_error(None)
    assert lib.flm_rotate_clip(None, x, 1, 16, 4, key, 1.0, x, cnt, s, S) == FLM_EINVAL
    assert lib.flm_l2_factors_dev(None, None, 16, 1, 16, 1.0, None, None, None, None) == FLM_EINVAL
    assert lib.flm_scale_rows_dev(None, None, 16, 1, 16, None, None, 16, None) == FLM_EINVAL
    assert lib.flm_rotate_clip_dev(None, None, 16, 1, 16, 4, None, None, None, 16, None, None) == FLM_EINVAL
    assert b"NULL" in lib.flm_last_error(None)
    v = lib.flm_version()
    assert all(w in v for w in (b"l2_clip", b"rotate", b"codec", b"0.4", b"gfx950"))


def test_engine_and_bindings_name_the_calls():
    import inspect
    import os
    import re
    from flamingo_amd import _lib
    from flamingo_amd.engine import MaskEngine
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "flamingo_hip.h")).read()
    util = open(os.path.join(root, "integration", "util_flm.py")).read()
    names = {"flm_l2_clip_check": 4, "flm_l2_factors_dev": 10, "flm_scale_rows_dev": 9, "flm_rotate_clip_dev": 12,
             "flm_l2_clip": 8, "flm_rotate_clip": 11}
    for name, n_args in names.items():
        assert re.search(r"\bint %s\(" % name, hdr) and len(_lib.SIGNATURES[name][1]) == n_args, name
    assert hdr.count("SA_ClientAgent.py:300-304") >= 6 + 3                      # every declaration cites it, as the rotation does
    assert len(_lib.SIGNATURES["flm_rotate_dev"][1]) == 12 and len(_lib.SIGNATURES["flm_rotate"][1]) == 9   # untouched
    for m in ("l2_clip_check", "l2_clip", "l2_factors_dev", "scale_rows_dev", "rotate_clip_dev"):
        assert callable(getattr(MaskEngine, m)), m
    assert inspect.signature(MaskEngine.rotate).parameters["clip_norm"].default is None
    for host in ("flm_l2_clip_check", "flm_l2_clip", "flm_rotate_clip", "flm_rotate"):
        assert '"%s"' % host in util
    for fn in ("l2_clip_check", "l2_clip", "rotate"):
        assert "def %s(" % fn in util
    assert "clip_norm=None" in util


# ------------------------------------------------------------------ the agents' options
def test_configure_l2_clip_refusals():
    from flamingo_amd.abides.flamingo import protocol as param
    try:
        param.configure(L=4001, codec=False)
        assert param.l2_clip() is None
        with pytest.raises(ValueError):
            param.configure(l2_clip=1.0)                          # needs the float inputs, as rotate and dp_noise do
        param.configure(l2_clip=0)                                # off needs nothing
        for bad in (-1.0, float("inf"), float("nan"), 1e-50, 1e39):  # the last two: 0 and inf as float32
            with pytest.raises(ValueError):
                param.configure(codec=(7, 1.0, "nearest"), l2_clip=bad)
        assert param.l2_clip() is None
        param.configure(codec=(7, 1.0, "stochastic", 2), rotate=5, l2_clip=2.28125)
        assert param.l2_clip() == 2.28125 and param.rotate_bits() == 5 and param.ring_len() == 2016
        param.configure(l2_clip=0.3)
        assert param.l2_clip() == float(np.float32(0.3))          # the float32 the library takes
        param.configure(rotate=0)
        assert param.l2_clip() == float(np.float32(0.3)) and param.ring_len() == 2001   # with and without the rotation
        param.configure(l2_clip=0)
        assert param.l2_clip() is None
        param.configure(l2_clip=1.5)
        param.configure(codec=False)                              # the float inputs off: the clip with them
        assert param.l2_clip() is None
        param.configure(codec=(7, 1.0, "nearest"))
        assert param.l2_clip() is None
    finally:
        param.configure(codec=False, L=param.P.vector_len)


def test_driver_option():
    from flamingo_amd.abides import config_flamingo as cfg
    _, args = cfg.parse(["-c", "flamingo", "--float_inputs", "7,1,sr,pack2", "--rotate", "5", "--l2_clip", "2.28125"])
    assert args.l2_clip == 2.28125 and args.rotate == 5
    assert cfg.parse(["-c", "flamingo"])[1].l2_clip == 0.0
    # the synthetic cohort of the agents' test straddles that norm
    from flamingo_amd.synthetic import float_update
    norms = np.array([_exact_norm(float_update(i, 4001, 1.0, 5)) for i in range(128)])
    assert norms.min() > 2.2 and norms.max() < 2.35 and 40 <= int((norms > 2.28125).sum()) <= 88
