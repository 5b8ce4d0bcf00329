"""The premises of tests/dp_cases.py, and the noise's entry points as far as they go without a GPU: the bounds of
Z, the block-interleaved layout and the mask of the last draw, the moments of the summed noise, and
flm_codec_check_noise against the restatement's rules at their edges."""
from __future__ import annotations

import ctypes

import numpy as np
import pytest

import codec_cases as K
import dp_cases as D
import pack_cases as PC
from codec_cases import oracle

FLM_EINVAL, FLM_ERANGE = -1, -4     # include/flamingo_hip.h


@pytest.fixture(scope="module")
def lib():
    from flamingo_amd import build, _lib
    build.build()
    return _lib.load()


# ------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("b", D.NOISE_BITS + (64, 256))
def test_noise_stays_within_half_the_coins(b):
    for L in (1, 16, 17, 2077):
        z = D.noise(D.seed(3), L, b)
        assert z.shape == (L,) and z.dtype == np.int64 and abs(z).max() <= b // 2
    assert not D.noise(D.seed(3), 33, 0).any()


@pytest.mark.parametrize("b", (2, 34, 64, 160))
def test_draws_are_block_interleaved(b):
    """Draw d of parameter block beta is block m beta + d of the stream, word l % 16 of it."""
    L, m = 100, D.draws(b)
    w = D.noise_words(D.seed(5), L, b)
    assert w.shape == (L, m)
    for beta in (0, 3, 6):
        for d in sorted({0, m - 1}):
            block = oracle.prg(D.seed(5), 16, slot0=16 * (m * beta + d))       # one whole ChaCha block
            if d == m - 1 and b % 32:
                block = block & np.uint32(2 ** (b % 32) - 1)
            n = min(16, L - 16 * beta)
            assert np.array_equal(w[16 * beta:16 * beta + n, d], block[:n]), (beta, d)


def test_last_draw_keeps_r_bits():
    for b in (2, 30, 34, 170):
        r = b % 32
        w = D.noise_words(D.seed(7), 4096, b)
        assert int(w[:, -1].max()) < 2 ** r and int(np.bitwise_or.reduce(w[:, -1])) == 2 ** r - 1
        if w.shape[1] > 1:
            assert int(w[:, 0].max()) >= 2 ** 31        # the draws before it are whole words
    assert int(D.noise_words(D.seed(7), 4096, 32)[:, -1].max()) >= 2 ** 31          # r = 0: no mask
    # the heads of all m draws are counted: Z + b / 2 is the popcount over every draw of the parameter
    w = D.noise_words(D.seed(7), 64, 160)
    assert np.array_equal(D.noise(D.seed(7), 64, 160) + 80, [sum(bin(int(v)).count("1") for v in row) for row in w])


@pytest.mark.parametrize("n,b", ((8, 2), (8, 34), (8, 64), (4, 256)))
def test_moments_of_the_summed_noise(n, b):
    """The sum over n clients is a centred Binomial(n b, 1/2): variance n b / 4.  L = 16384 samples: the variance
    estimator's relative standard deviation is sqrt(2 / L) = 1.1 %, so 5 % is 4.5 sigma; the seeds are fixed."""
    L = 16384
    z = sum(D.noise(D.seed(i), L, b) for i in range(n))
    var = n * b / 4.0
    ratio = float(np.mean(z.astype(np.float64) ** 2)) / var
    print(f"n = {n}, b = {b}: sample variance / expected = {ratio:.4f}, mean = {z.mean():.4f}")
    assert abs(ratio - 1.0) <= 0.05
    assert abs(float(z.mean())) <= 4.5 * np.sqrt(var / L)


def test_noised_fields_stay_within_zero_and_twice_the_noised_bias():
    for P, f, c, b in D.gpu_cases():
        if P == 1:
            continue
        x = K.random_row(2077, c, 11, wild=True)
        for dither in (None, K.DITHER):
            w, cl = D.encode_packed_noised(x, f, c, P, dither, D.seed(1), b)      # asserts 0 <= u <= 2 B_n
            assert cl.sum() == K.encode(x, f, c, dither)[1].sum() and len(w) == -(-2077 // P)
            plain = D.decode_packed_noised(w, 2077, f, c, P, b) * np.float32(2.0 ** f)
            q = K.encode(x, f, c, dither)[0].view(np.int32).astype(np.int64)
            assert np.array_equal(plain.astype(np.int64) - q, D.noise(D.seed(1), 2077, b))


def test_headroom_examples_and_edges():
    for f, c, P, b, n in D.HEADROOM_EXAMPLES + (D.UNPACKED_EDGE,):
        assert D.n_max(f, c, P, b) == n and D.headroom_ok(f, c, P, b, n) and not D.headroom_ok(f, c, P, b, n + 1)
    assert D.bias_n(4, 1.0, 30) == 31 and D.bias_n(2, 1.0, 2) == 5
    f, c, P, n = D.NO_ROOM
    assert D.headroom_ok(f, c, P, 0, n) and not D.headroom_ok(f, c, P, 2, n)
    for f, c, P, b, n, L in D.GPU_ROUNDS:
        assert D.headroom_ok(f, c, P, b, n) and D.length_ok(b, L)
    for P, f, c, b in D.gpu_cases():
        assert D.headroom_ok(f, c, P, b, 1)
    assert {P for P, *_ in D.gpu_cases()} == {1, 2, 4} and {b for *_, b in D.gpu_cases()} == set(D.NOISE_BITS)
    assert D.length_ok(64, 2 ** 35) and not D.length_ok(64, 2 ** 35 + 1)


# ------------------------------------------------------------------ the library, no device
def test_codec_check_noise_at_the_edges(lib):
    ck = lib.flm_codec_check_noise
    for f, c, P, b, n in D.HEADROOM_EXAMPLES + (D.UNPACKED_EDGE,):
        assert ck(f, c, P, b, n, 0) == 0 and ck(f, c, P, b, n + 1, 0) == FLM_ERANGE, (f, c, P, b, n)
    assert b"headroom" in lib.flm_last_error(None)
    f, c, P, n = D.NO_ROOM
    assert ck(f, c, P, 0, n, 0) == 0 and ck(f, c, P, 2, n, 0) == FLM_ERANGE
    # without noise the rule is the one there was
    assert ck(16, 4.0, 1, 0, 8191, 0) == lib.flm_codec_check(16, 4.0, 8191) == 0
    assert ck(16, 4.0, 1, 0, 8192, 0) == lib.flm_codec_check(16, 4.0, 8192) == FLM_ERANGE
    assert ck(7, 1.0, 2, 0, 256, 0) == lib.flm_codec_check_packed(7, 1.0, 2, 256) == FLM_ERANGE


def test_codec_check_noise_length_rule(lib):
    ck = lib.flm_codec_check_noise
    for b in (2, 64, 160, 1024):
        m = D.draws(b)
        blocks = 2 ** 32 // m                       # the most parameter blocks: m blocks <= 2^32
        L = 16 * blocks
        assert D.length_ok(b, L) and not D.length_ok(b, L + 1)
        assert ck(4, 1.0, 1, b, 1, L) == 0 and ck(4, 1.0, 1, b, 1, L + 1) == FLM_ERANGE, b
    assert 2 * (2 ** 35 // 16) == 2 ** 32           # b = 64: m ceil(L / 16) = 2^32 exactly, and one block above it
    assert ck(4, 1.0, 2, 64, 1, 2 ** 35) == 0 and ck(4, 1.0, 2, 64, 1, 2 ** 35 + 1) == FLM_ERANGE
    assert b"2^32" in lib.flm_last_error(None)
    assert ck(4, 1.0, 1, 0, 1, 2 ** 64 - 1) == 0    # no noise: no noise stream
    assert ck(4, 1.0, 1, 64, 1, 0) == 0             # L_params = 0: the headroom alone


def test_codec_check_noise_refusals(lib):
    ck = lib.flm_codec_check_noise
    for b in (1, 31, 1025, 1026, -2, -1):           # odd, beyond 1024, negative
        assert ck(4, 1.0, 2, b, 1, 0) == FLM_EINVAL, b
    assert b"noise_bits" in lib.flm_last_error(None)
    for pack in (0, 3, 8, -2):
        assert ck(4, 1.0, pack, 2, 1, 0) == FLM_EINVAL, pack
    assert b"pack" in lib.flm_last_error(None)
    for f, c in ((-1, 1.0), (31, 1.0), (7, 0.0), (7, -1.0), (7, float("inf")), (7, float("nan"))):
        for P in (1, 2):
            assert ck(f, c, P, 2, 1, 0) == FLM_EINVAL, (f, c, P)
    assert ck(4, 1.0, 2, 2, 0, 0) == FLM_EINVAL
    assert ck(4, 1.0, 1, 1024, 1, 0) == 0 and ck(2, 1.0, 4, 246, 1, 0) == 0 and ck(2, 1.0, 4, 248, 1, 0) == FLM_ERANGE


def test_codec_check_noise_agrees_with_the_restatement(lib):
    for P in (1, 2, 4):
        for f in (0, 2, 4, 7, 16):
            for c in (0.3, 1.0, 1.0000001, 4.0):
                for b in (0, 2, 30, 64, 246, 1024):
                    for n in (1, 25, 26, 255, 1057, 1058, 8176, 8177, 2 ** 20, 2 ** 31):
                        want = D.headroom_ok(f, c, P, b, n)
                        assert (lib.flm_codec_check_noise(f, c, P, b, n, 0) == 0) == want, (P, f, c, b, n)


def test_entry_points_reject_null_handles_and_bad_arguments(lib):
    x = (ctypes.c_float * 4)()
    w = (ctypes.c_uint32 * 4)()
    z = (ctypes.c_uint8 * 32)()
    seg = (ctypes.c_int64 * 2)(0, 0)
    assert lib.flm_client_encode_noise_mask(None, x, 1, seg, None, None, 4, 7, 1.0, 2, None, 2, z, w, None) == FLM_EINVAL
    assert b"NULL" in lib.flm_last_error(None)
    assert lib.flm_client_encode_noise_mask_dev(None, None, 4, 1, seg, None, None, 4, 7, 1.0, 2, None, 2, None, None, 4,
                                                None, None) == FLM_EINVAL
    assert lib.flm_decode_unpack_noise(None, w, 4, 7, 1.0, 2, 2, 1, x) == FLM_EINVAL
    assert lib.flm_decode_unpack_noise_dev(None, None, 4, 7, 1.0, 2, 2, 1, None, None) == FLM_EINVAL
    assert lib.flm_store_unmask_unpack_noise_f32(None, None, None, 0, 4, 4, 1.0, 2, 30, 1, x) == FLM_EINVAL
    assert lib.flm_store_unmask_unpack_noise_f32(None, None, None, 0, 4, 4, 1.0, 2, 31, 1, x) == FLM_EINVAL
    assert lib.flm_store_unmask_unpack_noise_f32(None, None, None, 0, 4, 4, 1.0, 2, 30, 1058, x) == FLM_ERANGE
    v = lib.flm_version()
    assert b"dp_noise" in v and b"pack" in v and b"0.4" in v and b"gfx950" in v


def test_engine_and_bindings_name_the_calls():
    import inspect
    import os
    import re
    from flamingo_amd import _lib
    from flamingo_amd.engine import MaskEngine
    from flamingo_amd.ingest import VectorStore
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "include", "flamingo_hip.h")) as fh:
        hdr = fh.read()
    with open(os.path.join(root, "integration", "util_flm.py")) as fh:
        util = fh.read()
    for name in ("flm_codec_check_noise", "flm_client_encode_noise_mask", "flm_client_encode_noise_mask_dev",
                 "flm_decode_unpack_noise", "flm_decode_unpack_noise_dev", "flm_store_unmask_unpack_noise_f32"):
        assert re.search(r"\bint %s\(" % name, hdr) and name in _lib.SIGNATURES, name
    for host in ("flm_client_encode_noise_mask", "flm_decode_unpack_noise"):
        assert len(_lib.SIGNATURES[host + "_dev"][1]) - len(_lib.SIGNATURES[host][1]) in (1, 3)  # stream (+ two pitches)
        assert '"%s"' % host in util
    for fn in ("codec_check_noise", "client_encode_noise_mask", "decode_unpack"):
        assert "def %s(" % fn in util
    assert callable(MaskEngine.client_encode_noise_mask) and callable(MaskEngine.client_encode_noise_mask_dev)
    for fn in (MaskEngine.codec_check, MaskEngine.decode_unpack, MaskEngine.decode_unpack_dev, VectorStore.unmask_unpack_f32):
        assert inspect.signature(fn).parameters["noise_bits"].default == 0
    assert inspect.signature(MaskEngine.codec_check).parameters["L"].default == 0
    assert PC.PACKS == (2, 4)
