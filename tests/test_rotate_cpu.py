"""The randomised block Hadamard rotation without a GPU: the premises of tests/rotate_cases.py (the restatement the
kernel is held to bit for bit by tests/test_rotate_gpu.py), the library's rule and refusals, and the agents' options."""
from __future__ import annotations

import ctypes

import numpy as np
import pytest

import rotate_cases as R
from codec_cases import oracle

FLM_EINVAL, FLM_ERANGE = -1, -4     # include/flamingo_hip.h


@pytest.fixture(scope="module")
def lib():
    from flamingo_amd import build, _lib
    build.build()
    return _lib.load()


# ------------------------------------------------------------------ the restatement
def test_sign_bit_convention_against_the_prg():
    L_rot = 96 + 16
    w = oracle.prg(R.KEY, 4)
    assert np.array_equal(R.sign_words(R.KEY, L_rot), w) and len(R.sign_words(R.KEY, 16)) == 1
    m = R.sign_mask(R.KEY, L_rot)
    for l in (0, 1, 31, 32, 33, 63, 64, 95, 111):
        assert int(m[l]) == ((int(w[l // 32]) >> (l % 32)) & 1) << 31, l
    assert 0 < int((m != 0).sum()) < L_rot
    assert not np.array_equal(m, R.sign_mask(R.KEY2, L_rot))
    # a flip is an XOR of the sign bit: -0.0 from +0.0, and a NaN keeps its payload
    v = np.array([0.0, 1.5, np.nan], np.float32)
    f = R._flip(v, np.full(3, 0x80000000, np.uint32))
    assert list(f.view(np.uint32)) == [0x80000000, 0xBFC00000, int(v.view(np.uint32)[2]) ^ 0x80000000]


def test_c_h_bit_patterns():
    for h in R.LOG2_BLOCKS:
        c = R.c_h(h)
        assert c.dtype == np.float32
        if h % 2 == 0:
            assert int(c.view(np.uint32)) == (127 - h // 2) << 23                       # 2^(-h / 2) exactly
        else:
            assert int(c.view(np.uint32)) == R.RSQRT2_BITS - (((h - 1) // 2) << 23)     # 0x3F3504F3 2^(-(h - 1) / 2)
        assert c == np.float32(2.0 ** (-h / 2.0))                                       # float32(2^(-h / 2)) either way
    assert R.RSQRT2_BITS == int(np.float32(np.sqrt(0.5)).view(np.uint32))


@pytest.mark.parametrize("h", R.LOG2_BLOCKS)
def test_forward_against_float64_hadamard_product(h):
    H = 1 << h
    x = np.random.default_rng(h).standard_normal(3 * H).astype(np.float32)
    y, bad = R.forward(x, R.KEY, h)
    assert bad == 0 and y.dtype == np.float32 and len(y) == 3 * H
    signed = R._flip(x, R.sign_mask(R.KEY, len(x))).astype(np.float64)
    want = R.hadamard64(signed, h)
    for b in range(3):
        blk = slice(b * H, (b + 1) * H)
        bound = R.error_bound(float(np.linalg.norm(x[blk].astype(np.float64))), h)
        assert np.max(np.abs(y[blk].astype(np.float64) - want[blk])) <= bound
    # inverse o forward within twice that bound (the second transform sees a block of the same norm)
    back = R.inverse(y, R.KEY, h, len(x))
    for b in range(3):
        blk = slice(b * H, (b + 1) * H)
        bound = 2 * R.error_bound(float(np.linalg.norm(x[blk].astype(np.float64))), h) * (1 + 2.0 ** -20)
        assert np.max(np.abs(back[blk].astype(np.float64) - x[blk])) <= bound


def test_stages_are_the_walsh_hadamard_butterflies():
    # h = 4 on unit vectors: column j of H_16 is (-1)^popcount(i & j), scaled by 1 / 4
    zero_key_mask = np.zeros(16, np.uint32)
    for j in (0, 1, 6, 15):
        e = np.zeros(16, np.float32)
        e[j] = 1.0
        y = R._stages(R._flip(e, zero_key_mask), 4)
        want = np.array([(-1) ** bin(i & j).count("1") for i in range(16)], np.float32) / 4
        assert np.array_equal(y, want)


def test_tail_reads_as_zero_and_lengths():
    for h in (4, 7, 12):
        H = 1 << h
        for L in R.lengths(h):
            assert R.rotated_len(L, h) % H == 0 and 0 <= R.rotated_len(L, h) - L < H
    x = R.rows(1, 37, 3)[0]
    padded = np.zeros(64, np.float32)
    padded[:37] = x
    assert np.array_equal(R.bits(R.forward(x, R.KEY, 5)[0]), R.bits(R.forward(padded, R.KEY, 5)[0]))
    assert len(R.inverse(R.forward(x, R.KEY, 5)[0], R.KEY, 5, 37)) == 37


def test_nonfinite_inputs_become_zero_and_are_counted():
    x = R.rows(1, 50, 4)[0]
    clean = x.copy()
    for l, v in ((0, np.nan), (15, np.inf), (16, -np.inf), (49, np.nan)):
        x[l], clean[l] = v, 0.0
    y, bad = R.forward(x, R.KEY, 4)
    y0, bad0 = R.forward(clean, R.KEY, 4)
    assert (bad, bad0) == (4, 0) and np.array_equal(R.bits(y), R.bits(y0)) and np.all(np.isfinite(y))
    # +0.0, not -0.0, before the flips: a block of one NaN alone is the block of +0.0
    z, _ = R.forward(np.array([np.nan] + [0.0] * 15, np.float32), R.KEY, 4)
    z0, _ = R.forward(np.zeros(16, np.float32), R.KEY, 4)
    assert np.array_equal(z.view(np.uint32), z0.view(np.uint32))
    # the inverse has no such handling
    assert np.isnan(R.inverse(np.array([np.inf] + [0.0] * 15, np.float32), R.KEY, 4, 16)).sum() == 0
    assert np.isnan(R.inverse(np.array([np.inf, -np.inf] + [0.0] * 14, np.float32), R.KEY, 4, 16)).any()


def test_one_hot_claim():
    c = R.ONE_HOT
    xs = R.one_hot_clients()
    exact = (xs.astype(np.float64).sum(axis=0) / len(xs)).astype(np.float32)
    key = R.KEY
    ys = np.stack([R.forward(x, key, c["h"])[0] for x in xs])
    mean_rot, clipped, qmax = R.codec_mean(ys, c["f"], c["c"], c["pack"])
    assert clipped == [0] * len(xs) and qmax == 16
    back = R.inverse(mean_rot, key, c["h"], c["L"])
    assert np.all(back == exact)                              # by value: -0.0 occurs
    plain, clipped, _ = R.codec_mean(xs, c["f"], c["c"], c["pack"])
    assert clipped == [1] * len(xs)
    assert float(exact[5]) - float(plain[5]) == 0.1875 and float(exact[5]) == 0.25


# ------------------------------------------------------------------ the library, no device
def test_rotate_check_values_and_refusals(lib):
    out = ctypes.c_uint64(0)
    for h in R.LOG2_BLOCKS:
        for L in R.lengths(h) + (4001,):
            assert lib.flm_rotate_check(L, h, ctypes.byref(out)) == 0 and out.value == R.rotated_len(L, h), (L, h)
    assert lib.flm_rotate_check(100, 6, None) == 0
    for h in (3, 13, 0, -1, 64):
        assert lib.flm_rotate_check(100, h, ctypes.byref(out)) == FLM_EINVAL, h
    assert b"log2_block" in lib.flm_last_error(None)
    assert lib.flm_rotate_check(0, 6, ctypes.byref(out)) == FLM_EINVAL
    # L_rot / 32 words of sign stream within the PRG's 2^36 slots: L_rot <= 2^41
    assert lib.flm_rotate_check(2 ** 41, 12, ctypes.byref(out)) == 0 and out.value == 2 ** 41
    assert lib.flm_rotate_check(2 ** 41 - 5, 4, ctypes.byref(out)) == 0 and out.value == 2 ** 41
    assert lib.flm_rotate_check(2 ** 41 + 1, 4, ctypes.byref(out)) == FLM_ERANGE
    assert b"2^36" in lib.flm_last_error(None)
    assert lib.flm_rotate_check(2 ** 64 - 1, 12, ctypes.byref(out)) == FLM_ERANGE
    assert lib.flm_rotate_check(2 ** 64 - 1, 3, ctypes.byref(out)) == FLM_EINVAL


def test_rotate_calls_reject_null_handles(lib):
    x = (ctypes.c_float * 16)()
    key = (ctypes.c_uint8 * 32)()
    cnt = (ctypes.c_uint32 * 1)()
    assert lib.flm_rotate(None, x, 1, 16, 4, key, 0, x, cnt) == FLM_EINVAL
    assert b"NULL" in lib.flm_last_error(None)
    assert lib.flm_rotate_dev(None, None, 16, 1, 16, 4, None, 0, None, 16, None, None) == FLM_EINVAL
    assert b"NULL" in lib.flm_last_error(None)
    v = lib.flm_version()
    assert b"rotate" in v and b"0.4" in v and b"gfx950" in v


def test_engine_and_bindings_name_the_calls():
    import os
    import re
    from flamingo_amd import _lib
    from flamingo_amd.engine import MaskEngine
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "flamingo_hip.h")).read()
    for name in ("flm_rotate_check", "flm_rotate_dev", "flm_rotate"):
        assert re.search(r"\bint %s\(" % name, hdr) and name in _lib.SIGNATURES, name
    assert len(_lib.SIGNATURES["flm_rotate_dev"][1]) == 12 and len(_lib.SIGNATURES["flm_rotate"][1]) == 9
    for m in ("rotate_check", "rotate", "rotate_dev"):
        assert callable(getattr(MaskEngine, m))


# ------------------------------------------------------------------ the agents' options
def test_configure_rotate_refusals_and_lengths():
    import hashlib
    from flamingo_amd.abides.flamingo import protocol as param
    root = bytes(range(32))
    try:
        param.configure(root=root, L=4001, codec=False)
        assert param.rotate_bits() == 0 and param.rotated_len() == 4001 and param.ring_len() == 4001
        with pytest.raises(ValueError):
            param.configure(rotate=5)                         # needs the float inputs, as dp_noise does
        for bad in (3, 13, -1, 1):
            with pytest.raises(ValueError):
                param.configure(codec=(7, 1.0, "nearest"), rotate=bad)
        for pack, words in ((1, 4032), (2, 2016), (4, 1008)):
            param.configure(codec=(7, 1.0, "stochastic", pack), rotate=5)
            assert param.rotate_bits() == 5 and param.rotated_len() == 4032 and param.ring_len() == words
            param.configure(rotate=0)
            assert param.rotate_bits() == 0 and param.rotated_len() == 4001 and param.ring_len() == -(-4001 // pack)
        param.configure(codec=(7, 1.0, "nearest"), rotate=12)
        assert param.rotated_len() == 4096
        assert param.rotation_key(3) == hashlib.sha256(b"flamingo rotation" + root + (3).to_bytes(8, "little")).digest()
        assert param.rotation_key(3) != param.rotation_key(4)
        param.configure(codec=False)                          # the float inputs off: the rotation with them
        assert param.rotate_bits() == 0 and param.ring_len() == 4001
    finally:
        param.configure(codec=False, L=param.P.vector_len)


def test_driver_option_and_synthetic_update():
    from flamingo_amd.abides import config_flamingo as cfg
    from flamingo_amd.synthetic import float_update
    _, args = cfg.parse(["-c", "flamingo", "--float_inputs", "7,1,sr,pack2", "--rotate", "5"])
    assert args.rotate == 5 and cfg.parse(["-c", "flamingo"])[1].rotate == 0
    for h in (4, 5, 12):
        x = float_update(3, 1000, 1.0, h)
        bound = 2.0 ** -((h + 1) // 2 + 1)
        assert x.dtype == np.float32 and np.max(np.abs(x)) <= bound
        y, bad = R.forward(x, R.KEY, h)
        assert bad == 0 and np.max(np.abs(y)) <= 0.5 * (1 + 2.0 ** -10)       # no rotated coordinate near the clip
    assert np.array_equal(float_update(3, 1000, 1.0), float_update(3, 1000, 1.0, 0))
