"""The premises of tests/pack_cases.py, and the packed codec's entry points as far as they go without a GPU:
|q| <= B under both roundings, the headroom edges, no word of a worst-case round's unreduced sum reaches 2^32,
the packed decode is the unpacked decode bit for bit, and flm_codec_check_packed decides the rule on the host."""
from __future__ import annotations

import ctypes

import numpy as np
import pytest

import codec_cases as K
import pack_cases as C

FLM_EINVAL, FLM_ERANGE = -1, -4     # include/flamingo_hip.h


@pytest.fixture(scope="module")
def lib():
    from flamingo_amd import build, _lib
    build.build()
    return _lib.load()


# ------------------------------------------------------------------ the restatement
def test_fields_stay_within_zero_and_twice_the_bias():
    """|q| <= B, so u = q + B is in [0, 2B], in nearest and stochastic rounding: the value rows (+-c, the floats
    beside it, infinities, NaN), the threshold row and wild random rows."""
    for f, c in C.VALUE_PARAMS + ((4, 1.0), (0, 1.0), (5, 1.3), (3, 0.7)):
        B = C.bias(f, c)
        rows = [K.value_row(f, c), K.random_row(4099, c, 7, wild=True), np.full(64, c, np.float32),
                np.full(64, -c, np.float32)]
        for x in rows:
            for dither in (None, C.DITHER, bytes(32)):
                u, _ = C.fields(x, f, c, dither)
                assert u.min() >= 0 and u.max() <= 2 * B, (f, c, dither is None)
        if float(np.float32(c)) * 2 ** f != B:
            continue
        v = K.value_row(f, c)               # c 2^f an integer: +-c are the extreme fields themselves, dither or not
        for dither in (None, C.DITHER):
            u, cl = C.fields(v, f, c, dither)
            assert list(u[8:10]) == [2 * B, 0] and not cl[8:10].any()
            assert list(u[12:16]) == [2 * B, 0] * 2 and cl[12:16].all()        # beyond c and +-inf clip to +-c
            assert u[16] == B and cl[16]                                       # NaN -> 0 -> the bias itself


def test_headroom_edges():
    for f, c, P, n in C.HEADROOM_EDGES:
        assert C.headroom_ok(f, c, P, n) and not C.headroom_ok(f, c, P, n + 1), (f, c, P, n)
    assert C.bias(7, 1.0) == 128 and C.bias(2, 1.0) == 4 and C.bias(4, 1.01) == 17
    assert not C.headroom_ok(7, 1.0, 4, 1)        # 2B = 256 does not fit 8 bits at all
    for f, c, P, n, L in C.WORST_ROUNDS:
        assert C.headroom_ok(f, c, P, n) and K.headroom_ok(f, c, n)


def test_packing_puts_consecutive_parameters_low_field_first():
    assert list(C.pack_fields([1, 2, 3], 2)) == [1 | 2 << 16, 3]
    assert list(C.pack_fields([1, 2, 3, 4, 5], 4)) == [1 | 2 << 8 | 3 << 16 | 4 << 24, 5]
    w, cl = C.encode_packed(np.array([1.0, -1.0, 0.0], np.float32), 7, 1.0, 2)
    assert list(w) == [256, 128] and not cl.any()             # 2B | 0 << 16; B, and the field past L holds 0
    assert list(C.decode_packed(w, 3, 7, 1.0, 2)) == [1.0, -1.0, 0.0]


@pytest.mark.parametrize("f,c,P,n,L", C.WORST_ROUNDS)
def test_worst_case_round_sums_without_a_carry_and_decodes_as_the_unpacked_codec(f, c, P, n, L):
    xs, dithers = C.worst_inputs(f, c, n, L)
    packed = np.zeros(-(-L // P), np.uint64)
    plain = np.zeros(L, np.uint64)
    for x, d in zip(xs, dithers):
        packed += C.encode_packed(x, f, c, P, d)[0]
        plain += K.encode(x, f, c, d)[0]
    assert int(packed.max()) < 2 ** 32                        # the unreduced sums: no word wraps the ring
    # every third client at +c: the low field of some word holds at least ceil(n / 3) 2B
    assert int((packed & (2 ** (32 // P) - 1)).max()) >= -(-n // 3) * 2 * C.bias(f, c)
    got = C.decode_packed(packed.astype(np.uint32), L, f, c, P, n)
    want = K.decode((plain & 0xFFFFFFFF).astype(np.uint32), f, n)
    assert got.dtype == np.float32 and got.tobytes() == want.tobytes()


def test_packed_decode_is_the_unpacked_decode_of_each_field():
    rng = np.random.default_rng(5)
    for P in C.PACKS:
        f, c = C.pack_params(P)
        B = C.bias(f, c)
        for count in C.decode_counts(P):
            for L in (1, P - 1 or 1, P, P + 1, 4 * P + 3, 1027):
                u = rng.integers(0, 2 * B * count + 1, size=L)
                S = C.pack_fields(u, P)
                want = K.decode(((u - count * B) & 0xFFFFFFFF).astype(np.uint32), f, count)
                assert C.decode_packed(S, L, f, c, P, count).tobytes() == want.tobytes()


def test_threshold_row_pins_the_dither_index():
    x, picks = C.threshold_row()
    assert len(picks) >= 4 and np.all(np.abs(x) < C.THRESHOLD_C)
    u, cl = C.fields(x, C.THRESHOLD_F, C.THRESHOLD_C, C.DITHER)
    B = C.bias(C.THRESHOLD_F, C.THRESHOLD_C)
    assert not cl.any()
    for l, r, thr, away in picks:
        assert float(x[l]) * 2.0 ** (32 + C.THRESHOLD_F) in (thr, -thr)          # exact: thr < 2^24
        assert abs(int(u[l]) - B) == (1 if away else 0), (l, r, thr, away)
    # the picked parameters fall into every field of either width
    for P in C.PACKS:
        assert {l % P for l, *_ in picks} == set(range(P))


# ------------------------------------------------------------------ the library, no device
def test_codec_check_packed_headroom(lib):
    ck = lib.flm_codec_check_packed
    for f, c, P, n in C.HEADROOM_EDGES:
        assert ck(f, c, P, n) == 0 and ck(f, c, P, n + 1) == FLM_ERANGE, (f, c, P, n)
    assert b"carry" in lib.flm_last_error(None)
    for pack in (0, 1, 3, 8, -2):
        assert ck(7, 1.0, pack, 1) == FLM_EINVAL, pack
    assert b"pack" in lib.flm_last_error(None)
    for f, c in ((-1, 1.0), (31, 1.0), (7, 0.0), (7, -1.0), (7, float("inf")), (7, float("nan"))):
        assert ck(f, c, 2, 1) == FLM_EINVAL, (f, c)
    assert ck(7, 1.0, 2, 0) == FLM_EINVAL and ck(7, 1.0, 4, 1) == FLM_ERANGE


def test_codec_check_packed_agrees_with_the_restatement(lib):
    for P in C.PACKS:
        for f in (0, 1, 2, 4, 6, 7, 8, 14, 15, 16):
            for c in (0.3, 1.0, 1.0000001, 1.9, 4.0, 100.0):
                for n in (1, 2, 15, 16, 31, 32, 127, 128, 255, 256, 2047, 2048, 32767, 32768, 2 ** 31):
                    assert (lib.flm_codec_check_packed(f, c, P, n) == 0) == C.headroom_ok(f, c, P, n), (P, f, c, n)


def test_entry_points_reject_null_handles_and_bad_arguments(lib):
    x = (ctypes.c_float * 4)()
    w = (ctypes.c_uint32 * 4)()
    seg = (ctypes.c_int64 * 2)(0, 0)
    assert lib.flm_client_encode_pack_mask(None, x, 1, seg, None, None, 4, 7, 1.0, 2, None, w, None) == FLM_EINVAL
    assert b"NULL" in lib.flm_last_error(None)
    assert lib.flm_client_encode_pack_mask_dev(None, None, 4, 1, seg, None, None, 4, 7, 1.0, 2, None, None, 4, None,
                                               None) == FLM_EINVAL
    assert lib.flm_decode_unpack(None, w, 4, 7, 1.0, 2, 1, x) == FLM_EINVAL
    assert lib.flm_decode_unpack_dev(None, None, 4, 7, 1.0, 2, 1, None, None) == FLM_EINVAL
    assert lib.flm_store_unmask_unpack_f32(None, None, None, 0, 4, 7, 1.0, 2, 1, x) == FLM_EINVAL
    assert lib.flm_store_unmask_unpack_f32(None, None, None, 0, 4, 7, 1.0, 3, 1, x) == FLM_EINVAL
    assert lib.flm_store_unmask_unpack_f32(None, None, None, 0, 4, 7, 1.0, 2, 256, x) == FLM_ERANGE
    v = lib.flm_version()
    assert b"pack" in v and b"codec" in v and b"0.4" in v and b"gfx950" in v
