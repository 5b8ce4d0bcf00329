"""The premises of tests/dgauss_cases.py and everything of the table-sampled noise that needs no GPU: the table builder
(flamingo_amd/dgauss.py) against float64 and its own exact moments, the sampler's restatement against those moments,
flm_codec_check_gauss and flm_dgauss_check_table at their edges by code and text, and protocol.configure's dp_gauss."""
from __future__ import annotations

import ctypes
import math
from fractions import Fraction

import numpy as np
import pytest

import dgauss_cases as G
import dp_cases as D

FLM_EINVAL, FLM_ERANGE = -1, -4     # include/flamingo_hip.h


@pytest.fixture(scope="module")
def lib():
    from flamingo_amd import build, _lib
    build.build()
    return _lib.load()


def _p64(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))


# ------------------------------------------------------------------ the table builder
@pytest.mark.parametrize("sigma,tau", G.REAL_TABLES)
def test_table_is_the_truncated_discrete_gaussian(sigma, tau):
    from flamingo_amd import dgauss
    t = dgauss.table(sigma, tau)
    assert t.dtype == np.uint64 and t.shape == (2 * tau,)
    assert np.all(t[1:] >= t[:-1])                                              # non-decreasing
    p = dgauss.pmf(t)
    assert len(p) == 2 * tau + 1 and sum(p) == 1
    unit = Fraction(1, 2 ** 64)
    for k in range(tau + 1):                                                    # symmetric to a unit of 2^-64 per entry
        assert abs(p[tau + k] - p[tau - k]) <= unit, k
    ks = np.arange(-tau, tau + 1, dtype=np.float64)
    w = np.exp(-ks * ks / (2.0 * sigma * sigma))
    want = w / w.sum()
    for c in range(2 * tau + 1):
        assert abs(float(p[c]) - want[c]) <= 2.0 ** -50 * want[c] + 2.0 ** -63, c
    mean, var = dgauss.moments(t)
    assert isinstance(mean, Fraction) and isinstance(var, Fraction)
    assert abs(mean) <= Fraction(tau * (tau + 1), 2) * unit                     # sum_k k |p(k) - p(-k)|, k = 1..tau
    want_var = float((ks * ks * w).sum() / w.sum())
    assert abs(float(var) - want_var) <= 1e-12 * want_var
    # the off-by-one of the rule: table[0] is the chance of -tau, not 0
    assert t[0] > 0 or want[0] < 2.0 ** -64
    assert p[0] == Fraction(int(t[0]), 2 ** 64) and p[-1] == 1 - Fraction(int(t[-1]), 2 ** 64)


def test_tail_mass_and_the_default_tail():
    from flamingo_amd import dgauss
    assert 0.0 < dgauss.tail_mass(3.2, 32) < 2.0 ** -64
    # against the float64 sum where that still resolves the tail
    ks = np.arange(-400, 401, dtype=np.float64)
    w = np.exp(-ks * ks / (2.0 * 3.2 * 3.2))
    assert math.isclose(dgauss.tail_mass(3.2, 8), float(w[np.abs(ks) > 8].sum() / w.sum()), rel_tol=1e-12)
    assert dgauss.tail_mass(0.5, 0) == pytest.approx(1.0 - 1.0 / float(np.exp(-np.arange(-40, 41.0) ** 2 / 0.5).sum()), rel=1e-12)
    assert dgauss.default_tail(3.2) == 32 and dgauss.default_tail(0.5) == 5 and dgauss.default_tail(51.2) == 512
    assert dgauss.default_tail(51.3) == 513
    for bad in ((0.0, 5), (-1.0, 5), (float("nan"), 5), (float("inf"), 5), (1.0, 0), (1.0, 513), (1.0, 2.5)):
        with pytest.raises(ValueError):
            dgauss.table(*bad)
    with pytest.raises(ValueError):
        dgauss.moments(np.array([5, 4], np.uint64))


def test_coin_table_pins_the_off_by_one():
    """tau = 1 with [2^63, 2^63]: the count is 0 below 2^63 and 2 from it on, so z is -1 or +1 and never 0; and the
    table of a law on {-1, 0, 1} has table[0] = 2^64 P(Z = -1), not 0."""
    from flamingo_amd import dgauss
    z = G.noise(D.seed(9), 4096, G.coin())
    u = G.draws_u64(D.seed(9), 4096)
    assert set(np.unique(z)) == {-1, 1} and np.array_equal(z > 0, u >= np.uint64(2 ** 63))
    assert dgauss.moments(G.coin()) == (0, 1)
    t = dgauss.table(1.0, 1)
    p = dgauss.pmf(t)
    assert int(t[0]) > 0 and abs(float(p[0]) - math.exp(-0.5) / (1 + 2 * math.exp(-0.5))) < 1e-15
    assert not (G.noise(D.seed(9), 4096, G.all_zeros(3)) != 3).any() and not (G.noise(D.seed(9), 4096, G.all_ones(3)) != -3).any()


# ------------------------------------------------------------------ the sampler's restatement
def test_draws_are_the_binomial_stream_at_two_draws():
    from codec_cases import oracle
    L = 100
    u = G.draws_u64(D.seed(5), L)
    for beta in (0, 3, 6):
        hi = oracle.prg(D.seed(5), 16, slot0=16 * (2 * beta)).astype(np.uint64)
        lo = oracle.prg(D.seed(5), 16, slot0=16 * (2 * beta + 1)).astype(np.uint64)
        n = min(16, L - 16 * beta)
        assert np.array_equal(u[16 * beta:16 * beta + n], ((hi << np.uint64(32)) | lo)[:n])


def test_sample_variance_matches_the_table():
    """One fixed seed, sigma = 3.2, tau = 32, 2^16 samples.  The sample variance (about the known mean, 0 to 2^-54) has
    standard error sqrt((mu_4 - var^2) / n), mu_4 and var exact from the table; 5 standard errors."""
    from flamingo_amd import dgauss
    sigma, tau = 3.2, 32
    n = 2 ** 16
    t = dgauss.table(sigma, tau)
    z = G.noise(D.seed(2021), n, t)
    assert z.shape == (n,) and np.abs(z).max() <= tau
    mean, var = dgauss.moments(t)
    mu4 = dgauss.fourth_central_moment(t)
    se = math.sqrt(float(mu4 - var * var) / n)
    sample = float(np.mean(z.astype(np.float64) ** 2))
    print(f"sample variance {sample:.5f}, table variance {float(var):.5f}, standard error {se:.5f}, "
          f"off by {(sample - float(var)) / se:+.2f} standard errors; sample mean {z.mean():+.5f}")
    assert abs(sample - float(var)) <= 5.0 * se
    assert abs(float(z.mean())) <= 5.0 * math.sqrt(float(var) / n)
    assert abs(float(var) - sigma * sigma) < 1e-9 * sigma * sigma          # tau = 10 sigma: the truncation is invisible


def test_case_lists_hold():
    for f, c, P, tau, n in G.HEADROOM_EXAMPLES:
        assert G.n_max(f, c, P, tau) == n and G.headroom_ok(f, c, P, tau, n) and not G.headroom_ok(f, c, P, tau, n + 1)
    assert G.bias_n(4, 1.0, 15) == 31
    assert [p for p in G.gpu_params(512)] == [(1, 7, 1.0), (1, 2, 1.0), (2, 7, 1.0), (2, 2, 1.0)]
    assert (4, 2, 1.0) in G.gpu_params(G.ODD_TAU) and (4, 7, 1.0) not in G.gpu_params(1)
    t = G.even_steps()
    assert len(t) == 74 and np.all(t[1:] > t[:-1])
    assert set(G.counts(D.seed(1), 2077, t)) == set(range(75))              # every count and so every bisection leaf
    for tab in (G.low_word_table(0x12345678), G.top_bit_table()):
        assert np.all(tab[1:] > tab[:-1])
    assert len({int(v) >> 32 for v in G.low_word_table(0x12345678)}) == 1
    assert G.length_ok(2 ** 35) and not G.length_ok(2 ** 35 + 1)


# ------------------------------------------------------------------ the library, no device
def test_codec_check_gauss_headroom_is_the_binomial_rule_at_half_the_coins(lib):
    ck = lib.flm_codec_check_gauss
    for (f, c, P, tau, n), (_, _, _, b, nb) in zip(G.HEADROOM_EXAMPLES, D.HEADROOM_EXAMPLES + (D.UNPACKED_EDGE,)):
        assert n == nb and tau == b // 2
        assert ck(f, c, P, tau, n, 0) == 0 and ck(f, c, P, tau, n + 1, 0) == FLM_ERANGE, (f, c, P, tau, n)
        assert lib.flm_codec_check_noise(f, c, P, b, n, 0) == 0 and lib.flm_codec_check_noise(f, c, P, b, n + 1, 0) == FLM_ERANGE
    assert ck(4, 1.0, 2, 15, 1058, 0) == FLM_ERANGE and b"headroom" in lib.flm_last_error(None)
    f, c, P, n = D.NO_ROOM
    assert ck(f, c, P, 1, n, 0) == FLM_ERANGE
    for P in (1, 2, 4):
        for f in (0, 2, 4, 7, 16):
            for c in (0.3, 1.0, 1.0000001, 4.0):
                for tau in (1, 15, 32, 123, 124, 512):
                    for n in (1, 25, 26, 255, 1057, 1058, 8176, 8177, 2 ** 20, 2 ** 31):
                        assert (ck(f, c, P, tau, n, 0) == 0) == G.headroom_ok(f, c, P, tau, n), (P, f, c, tau, n)


def test_codec_check_gauss_refusals_and_length(lib):
    ck = lib.flm_codec_check_gauss
    for tau in (0, 513, -1, 1024):
        assert ck(4, 1.0, 2, tau, 1, 0) == FLM_EINVAL, tau
        assert lib.flm_last_error(None) == b"tail must be in 1..512"
    assert ck(4, 1.0, 2, 1, 1, 0) == 0 and ck(4, 1.0, 2, 512, 1, 0) == 0
    for pack in (0, 3, 8, -2):
        assert ck(4, 1.0, pack, 2, 1, 0) == FLM_EINVAL, pack
    assert b"pack" in lib.flm_last_error(None)
    for f, c in ((-1, 1.0), (31, 1.0), (7, 0.0), (7, -1.0), (7, float("inf")), (7, float("nan"))):
        for P in (1, 2):
            assert ck(f, c, P, 2, 1, 0) == FLM_EINVAL, (f, c, P)
    assert ck(4, 1.0, 2, 2, 0, 0) == FLM_EINVAL
    assert ck(2, 1.0, 4, 123, 1, 0) == 0 and ck(2, 1.0, 4, 124, 1, 0) == FLM_ERANGE
    # two blocks per parameter block: 2 ceil(L / 16) <= 2^32, whatever the tail
    for tau in (1, 32, 512):
        assert ck(4, 1.0, 1, tau, 1, 2 ** 35) == 0 and ck(4, 1.0, 1, tau, 1, 2 ** 35 + 1) == FLM_ERANGE, tau
    assert b"2^32" in lib.flm_last_error(None)
    assert ck(4, 1.0, 1, 32, 1, 0) == 0


def test_dgauss_check_table(lib):
    ck = lib.flm_dgauss_check_table
    for sigma, tau in G.REAL_TABLES:
        assert ck(_p64(G.real_table(sigma, tau)), tau) == 0
    for t in (G.all_zeros(3), G.all_ones(3), G.coin(), G.even_steps(), G.top_bit_table()):
        assert ck(_p64(t), len(t) // 2) == 0
    down = G.even_steps().copy()
    down[40] = down[39] - np.uint64(1)
    assert ck(_p64(down), G.ODD_TAU) == FLM_EINVAL and lib.flm_last_error(None) == b"the table must be non-decreasing"
    assert ck(_p64(down), 20) == 0                                   # the first 40 entries are in order
    top = np.array([2 ** 63, 2 ** 63 - 1], np.uint64)                # a decrease across bit 63: the compare is unsigned
    assert ck(_p64(top), 1) == FLM_EINVAL
    assert ck(None, 3) == FLM_EINVAL and b"NULL" in lib.flm_last_error(None)
    for tau in (0, 513, -1):
        assert ck(_p64(G.all_zeros(4)), tau) == FLM_EINVAL and lib.flm_last_error(None) == b"tail must be in 1..512"


def test_entry_points_reject_null_handles_and_name_the_feature(lib):
    x = (ctypes.c_float * 4)()
    w = (ctypes.c_uint32 * 4)()
    z = (ctypes.c_uint8 * 32)()
    seg = (ctypes.c_int64 * 2)(0, 0)
    t = G.coin()
    assert lib.flm_client_encode_gauss_mask(None, x, 1, seg, None, None, 4, 7, 1.0, 2, None, 1, _p64(t), z, w, None) == FLM_EINVAL
    assert b"NULL" in lib.flm_last_error(None)
    assert lib.flm_client_encode_gauss_mask_dev(None, None, 4, 1, seg, None, None, 4, 7, 1.0, 2, None, 1, None, None, None, 4,
                                                None, None) == FLM_EINVAL
    assert b"dp_gauss" in lib.flm_version() and b"dp_noise" in lib.flm_version()
    from flamingo_amd.engine import MaskEngine
    for fn in ("codec_check_gauss", "client_encode_gauss_mask", "client_encode_gauss_mask_dev"):
        assert callable(getattr(MaskEngine, fn))


# ------------------------------------------------------------------ the agents' configuration
def test_configure_refusals_and_off_means_off():
    from flamingo_amd.abides.flamingo import protocol as param
    from flamingo_amd.abides import config_flamingo
    param.configure(codec=False)
    try:
        before = (param.codec(), param.codec_pack(), param.codec_noise_bits(), param.rotate_bits(), param.round_bound())
        assert param.dp_gauss() is None and param.decode_noise_bits() == 0
        with pytest.raises(ValueError, match="float inputs"):
            param.configure(dp_gauss=(3.2, 32))                              # without the codec
        param.configure(codec=(4, 1.0, "stochastic", 2), dp_noise=30)
        assert param.decode_noise_bits() == 30 and param.dp_gauss() is None
        with pytest.raises(ValueError, match="dp_noise"):
            param.configure(dp_gauss=(3.2, 32))                              # with the binomial noise
        param.configure(dp_noise=0)
        with pytest.raises(ValueError, match="512"):
            param.configure(dp_gauss=51.3)                                   # default tail ceil(513) > 512
        with pytest.raises(ValueError):
            param.configure(dp_gauss=(3.2, 0))
        with pytest.raises(ValueError):
            param.configure(dp_gauss=(-1.0, 5))
        assert param.dp_gauss() is None
        param.configure(dp_gauss=3.2)
        assert param.dp_gauss() == (3.2, 32) and param.decode_noise_bits() == 64 and param.codec_noise_bits() == 0
        from flamingo_amd import dgauss
        assert np.array_equal(param.dp_gauss_table(), dgauss.table(3.2, 32))
        with pytest.raises(ValueError, match="dp_gauss"):
            param.configure(dp_noise=30)                                     # the other way round
        param.configure(dp_gauss=(0.5, 7))
        assert param.dp_gauss() == (0.5, 7) and len(param.dp_gauss_table()) == 14
        param.configure(dp_gauss=False)
        assert param.dp_gauss() is None and param.dp_gauss_table() is None and param.decode_noise_bits() == 0
        param.configure(dp_gauss=(3.2, 32))
        param.configure(codec=False)                                         # what it stands on turned off
        assert param.dp_gauss() is None
        assert (param.codec(), param.codec_pack(), param.codec_noise_bits(), param.rotate_bits(), param.round_bound()) == before
    finally:
        param.configure(codec=False)
    assert config_flamingo.parse_dp_gauss(None) is None and config_flamingo.parse_dp_gauss("3.2") == (3.2, 32)
    assert config_flamingo.parse_dp_gauss("3.2,40") == (3.2, 40)
    for bad in ("3.2,4,5", "x", "3.2,1.5"):
        with pytest.raises(SystemExit):
            config_flamingo.parse_dp_gauss(bad)
