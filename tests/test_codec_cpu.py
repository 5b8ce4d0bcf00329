"""The premises of tests/codec_cases.py, and the codec's entry points as far as they go without a GPU:
flm_codec_check decides the headroom rule on the host, and every new entry point refuses a NULL handle or a
bad parameter before any device call."""
from __future__ import annotations

import ctypes

import numpy as np
import pytest

import codec_cases as C

FLM_EINVAL, FLM_ERANGE = -1, -4     # include/flamingo_hip.h


@pytest.fixture(scope="module")
def lib():
    from flamingo_amd import build, _lib
    build.build()
    return _lib.load()


# ------------------------------------------------------------------ the restatement
def test_ties_round_to_even():
    for f, c in C.PARAMS:
        x = np.array([t * 2.0 ** -f for t, _ in C.TIES], np.float32)
        w, cl = C.encode(x, f, c)
        assert list(w.view(np.int32)) == [q for _, q in C.TIES] and not cl.any()


def test_value_rows_hold_what_they_claim():
    for f, c in C.PARAMS:
        x = C.value_row(f, c)
        w, cl = C.encode(x, f, c)
        top = int(np.float32(c) * 2.0 ** f)
        assert w[0] == 0 and w[1] == 0 and np.signbit(x[1])                  # -0.0 encodes to 0
        assert np.all(w[2:8] == 0) and np.all(x[2:6] != 0) and np.all(np.abs(x[2:6]) < 1.1754944e-38)  # subnormals
        assert list(w[8:10].view(np.int32)) == [top, -top] and not cl[8:10].any()       # +-c: not clipped
        assert not cl[10:12].any() and cl[12:16].all() and cl[16] and cl[17:19].all()   # inside / outside, inf, NaN
        assert list(w[12:16].view(np.int32)) == [top, -top, top, -top] and w[16] == 0
        assert C.headroom_ok(f, c, 1)
        # stochastic rounding of the same row stays within one step of the exact value, on the clipped value's side
        ws, cls = C.encode(x, f, c, C.DITHER)
        assert np.array_equal(cl, cls)
        assert np.all(np.abs(ws.view(np.int32).astype(np.int64) - w.view(np.int32).astype(np.int64)) <= 1)


def test_fraction_and_threshold_are_exact():
    rng = np.random.default_rng(5)
    t = (rng.random(4096) * 64.0 - 32.0).astype(np.float32)
    ti = np.trunc(t)
    fr = np.abs(t - ti).astype(np.float32)
    assert np.all(fr.astype(np.float64) == np.abs(t.astype(np.float64) - ti.astype(np.float64)))   # no rounding
    thr = np.trunc(fr.astype(np.float64) * 2.0 ** 32)
    big = fr >= 2.0 ** -8
    assert big.sum() > 3000 and np.all(thr[big] / 2.0 ** 32 == fr[big].astype(np.float64))
    assert np.all(thr < 2.0 ** 32) and np.float32(1.0) - np.float32(2.0 ** -24) == np.nextafter(np.float32(1), np.float32(0))
    # 16 steps of 2^-26 on top of 1/8 (the binade whose float32 spacing is 2^-26) are exact
    for k in range(17):
        assert float(np.float32(0.125 + k * 2.0 ** -26)) == 0.125 + k * 2.0 ** -26


def test_threshold_row_straddles_the_threshold():
    x, picks = C.threshold_row()
    assert len(picks) >= 4
    assert any(away for *_, away in picks) and any(not away for *_, away in picks)
    r = C.oracle.prg(C.DITHER, C.THRESHOLD_L)
    w, cl = C.encode(x, C.THRESHOLD_F, C.THRESHOLD_C, C.DITHER)
    assert not cl.any()
    for l, rl, thr, away in picks:
        assert int(r[l]) == rl and 0 < rl < 2 ** 24
        t = np.float32(x[l]) * np.float32(2.0 ** C.THRESHOLD_F)
        assert abs(float(t)) * 2.0 ** 32 == thr                          # the float hits the threshold exactly
        assert rl == (thr - 1 if away else thr)
        assert int(w.view(np.int32)[l]) == (int(np.sign(t)) if away else 0)
    # the words are the stream oracle.prg gives: a different seed moves the roundings
    w2, _ = C.encode(x, C.THRESHOLD_F, C.THRESHOLD_C, bytes(32))
    assert not np.array_equal(w, w2)


def test_stochastic_rounding_is_unbiased_on_average():
    x = np.full(1 << 16, 0.3 * 2.0 ** -4, np.float32)
    w, _ = C.encode(x, 4, 1.0, C.DITHER)
    q = w.view(np.int32)
    assert set(np.unique(q)) == {0, 1}
    t = float(np.float32(x[0]) * np.float32(16.0))
    assert abs(q.mean() - t) < 4 * np.sqrt(t * (1 - t) / q.size)         # four standard deviations


def test_decode_cases():
    i32 = [0, 1, -1, 2 ** 31 - 1, -2 ** 31, 2 ** 24 + 1]
    for f in (0, 16, 30):
        for n in C.DECODE_COUNTS:
            got = C.decode(C.DECODE_WORDS, f, n)
            assert got.dtype == np.float32
            for g, v in zip(got, i32):
                assert g == np.float32(np.float64(v) / (np.float64(n) * 2.0 ** f))
    assert C.decode(C.DECODE_WORDS, 0, 1)[5] == np.float32(2 ** 24)      # 2^24 + 1 rounds to even: one rounding
    assert C.decode(C.DECODE_WORDS, 0, 3)[1] == np.float32(1 / 3)
    # encode, sum, decode: the mean of values on the grid comes back exactly
    x = np.array([[0.5, -1.25, 3.0], [1.5, 0.25, -3.0]], np.float32)
    s = (C.encode(x[0], 8, 4.0)[0].astype(np.uint64) + C.encode(x[1], 8, 4.0)[0]).astype(np.uint32)
    assert list(C.decode(s, 8, 2)) == [1.0, -0.5, 0.0]


# ------------------------------------------------------------------ the library, no device
def test_codec_check_headroom(lib):
    ck = lib.flm_codec_check
    assert ck(30, 1.0, 1) == 0 and ck(30, 1.0, 2) == FLM_ERANGE
    assert ck(0, 2147483520.0, 1) == 0 and ck(0, 2.0 ** 31, 1) == FLM_ERANGE
    assert b"wrap" in lib.flm_last_error(None)
    for f, c in ((-1, 1.0), (31, 1.0), (16, 0.0), (16, -1.0), (16, float("inf")), (16, float("nan"))):
        assert ck(f, c, 1) == FLM_EINVAL, (f, c)
    assert ck(16, 4.0, 0) == FLM_EINVAL and ck(16, 4.0, -3) == FLM_EINVAL


def test_codec_check_agrees_with_the_restatement(lib):
    for f in (0, 1, 15, 16, 29, 30):
        for c in (1e-45, 0.3, 1.0, 1.0000001, 4.0, 1000.0, 32767.5, 2147483520.0, 3.0e38):
            for n in (1, 2, 3, 128, 8191, 8192, 2 ** 31 - 1, 2 ** 31, 2 ** 62):
                assert (lib.flm_codec_check(f, c, n) == 0) == C.headroom_ok(f, c, n), (f, c, n)


def test_entry_points_reject_null_handles_and_bad_arguments(lib):
    """A NULL context or store is an FLM_EINVAL with a message, before any device call."""
    x = (ctypes.c_float * 4)()
    w = (ctypes.c_uint32 * 4)()
    seg = (ctypes.c_int64 * 2)(0, 0)
    assert lib.flm_client_encode_mask(None, x, 1, seg, None, None, 4, 16, 4.0, None, w, None) == FLM_EINVAL
    assert b"NULL" in lib.flm_last_error(None)
    assert lib.flm_client_encode_mask_dev(None, None, 4, 1, seg, None, None, 4, 16, 4.0, None, None, 4, None,
                                          None) == FLM_EINVAL
    assert lib.flm_decode_sum(None, w, 4, 16, 1, x) == FLM_EINVAL
    assert lib.flm_decode_sum_dev(None, None, 4, 16, 1, None, None) == FLM_EINVAL
    assert lib.flm_store_unmask_f32(None, None, None, 0, 16, 1, x) == FLM_EINVAL
    assert lib.flm_store_unmask_f32(None, None, None, 0, 31, 1, x) == FLM_EINVAL
    assert lib.flm_store_unmask_f32(None, None, None, 0, 16, 0, x) == FLM_EINVAL
    assert b"codec" in lib.flm_version() and b"0.4" in lib.flm_version() and b"gfx950" in lib.flm_version()
