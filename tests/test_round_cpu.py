"""Conditional stochastic rounding without a GPU: the premises of tests/round_cases.py (the restatement the kernels are
held to bit for bit by tests/test_round_gpu.py), flm_round_bound bit for bit against its float64 sequence and against
exact rationals, every refusal of flm_round_check and flm_round_bound, and the agents' options."""
from __future__ import annotations

import ctypes
import math
from fractions import Fraction

import numpy as np
import pytest

import codec_cases as CC
import round_cases as RC

FLM_EINVAL, FLM_ERANGE = -1, -4     # include/flamingo_hip.h


@pytest.fixture(scope="module")
def lib():
    from flamingo_amd import build, _lib
    build.build()
    return _lib.load()


def _bound(lib, C, f, d, k):
    out = ctypes.c_uint64(0xDEAD)
    rc = lib.flm_round_bound(C, f, d, k, ctypes.byref(out))
    return rc, int(out.value)


# ------------------------------------------------------------------ the restatement and its lists
def test_restatement_is_the_codecs_encode_as_integers():
    x = np.array([0.26, -0.26, 3.0, -np.inf, np.nan, 0.0], np.float32)
    for s in (RC.seed("a"), RC.seed("b")):
        qs = RC.q(x, 2, 1.0, s)
        assert qs.dtype == np.int32 and qs[2] == 4 and qs[3] == -4 and qs[4] == 0 and qs[5] == 0   # +-Inf clips to +-c
        assert {int(qs[0]), -int(qs[1])} <= {1, 2}
        assert RC.sumsq(x, 2, 1.0, s) == sum(int(v) ** 2 for v in qs) and isinstance(RC.sumsq(x, 2, 1.0, s), int)
    assert RC.select([5, 3, 9], 2) == 3 and RC.select([5, 3, 9], 3) == 1 and RC.select([5, 3, 9], 5) == 0
    assert RC.select([5, 3, 9], 4) == 1 and RC.select([7], 7) == 0 and RC.select([7], 6) == 1
    f, c, xw, want = RC.WRAP_GUARD
    assert RC.sumsq(xw, f, c, RC.seed("w")) == want == 3 * 2 ** 60 and want * 6 > 2 ** 64 > want * 5


def test_threshold_row_flips_q_between_two_candidates():
    x, picks, cands = RC.threshold_case()
    assert len(picks) >= 4 and bytes(cands[1]) == CC.DITHER
    f, c = CC.THRESHOLD_F, CC.THRESHOLD_C
    under = RC.q(x, f, c, CC.DITHER)
    others = [RC.q(x, f, c, bytes(cands[k])) for k in (0, 2)]
    flipped = 0
    for l, r, thr, away in picks:
        # under DITHER the slot's word is r: one below the threshold rounds away from zero, at it truncates
        assert abs(int(under[l])) == (1 if away else 0), (l, away)
        flipped += any(int(o[l]) != int(under[l]) for o in others)
    assert flipped >= 2                               # the same parameter rounds differently under another candidate
    # a threshold of about 2^-8 or less: under a seed that is not DITHER nearly every picked slot truncates
    assert sum(abs(int(others[0][l])) for l, _, _, _ in picks) < sum(1 for p in picks if p[3])
    Q = [RC.sumsq(x, f, c, bytes(k)) for k in cands]
    assert len(set(Q)) == 3                           # and the sums tell the candidates apart


def test_case_lists_cover_what_they_claim():
    names = [n for n, *_ in RC.cases()]
    assert "threshold" in names and len(set(names)) == len(names)
    for f, c in CC.PARAMS:                            # every value of every value row, in pieces the rule admits
        pieces = [x for n, ff, cc, x, _ in RC.cases() if n.startswith(f"values f={f} ")]
        assert np.concatenate(pieces).tobytes() == CC.value_row(f, c).tobytes()
    assert RC.max_len(30, 1.0) == 15 and sum(n.startswith("values f=30") for n in names) == 3
    for name, f, c, x, cands in RC.cases():
        assert cands.shape == (8, 32) and x.dtype == np.float32 and 0 < len(x) <= RC.max_len(f, c)
        Q = [RC.sumsq(x, f, c, bytes(k)) for k in cands]
        B = math.ceil(Fraction(float(np.float32(c))) * 2 ** f)
        assert max(Q) <= len(x) * B * B < 2 ** 64, name
    assert RC.LENGTHS == (1, 15, 16, 17, 4095, 4096, 4097, 8193, 64 * 4096 + 5)
    rows = RC.random_rows(3, 4097, 1.0, 1)
    assert np.isnan(rows).any() and np.isinf(rows).any() and (np.abs(rows[np.isfinite(rows)]) > 1.0).any()
    assert rows[0].tobytes() != rows[1].tobytes()


# ------------------------------------------------------------------ the bound
def test_round_bound_matches_its_float64_sequence(lib):
    branches = set()
    for C, f, d, k in RC.BOUND_GRID:
        rc, got = _bound(lib, C, f, d, k)
        assert rc == 0 and got == RC.bound(C, f, d, k), (C, f, d, k, got)
        branches.add(RC.bound_branch(C, f, d, k))
    assert branches == {1, 2}                         # both sides of the min
    assert all(any((C, f, d) == g[:3] and g[3] in (1.0, RC.tail_of(0.1)) for g in RC.BOUND_GRID) for C, f, d in RC.SIMULATED)
    # the output pointer is optional
    assert lib.flm_round_bound(1.0, 0, 1, 0.0, None) == 0


def test_round_bound_lies_between_the_clipped_norm_and_the_worst_case():
    for C, f, d, k in RC.BOUND_GRID:
        got = RC.bound(C, f, d, k)
        s = Fraction(float(np.float32(C))) * 2 ** f * (1 + Fraction(1, 2 ** 19))
        # floor() takes at most 1 off, and the float64 evaluation errs by a few ulps of the result
        slack = 1 + Fraction(got, 2 ** 48)
        assert got + slack >= s * s, (C, f, d, k)
        r = math.isqrt(d)
        top = (s + r + 1) ** 2 if r * r != d else (s + r) ** 2
        assert got <= top + slack, (C, f, d, k)
        exact_b2 = s * s + Fraction(d, 4) + Fraction(k) * (s + Fraction(math.sqrt(d)) / 2)
        if RC.bound_branch(C, f, d, k) == 2:
            assert abs(got - exact_b2) <= slack + Fraction(k) * Fraction(math.sqrt(d)) / 2 ** 52, (C, f, d, k)
    # the tail widens it, never beyond the worst case
    C, f, d = RC.SIMULATED[0]
    seq = [RC.bound(C, f, d, k) for k in (0.0, 0.5, 1.0, 2.0, 10.0, 1e3, 1e9)]
    assert seq == sorted(seq) and seq[0] < seq[2] < seq[-1] == seq[-2]


def test_round_bound_refusals(lib):
    inf, nan = float("inf"), float("nan")
    for C in (0.0, -1.0, inf, nan, 1e-50, 1e39):      # the last two: 0 and inf as float32
        assert _bound(lib, C, 7, 16, 1.0) == (FLM_EINVAL, 0xDEAD), C
    for f in (-1, 31):
        assert _bound(lib, 1.0, f, 16, 1.0)[0] == FLM_EINVAL
    assert _bound(lib, 1.0, 7, 0, 1.0)[0] == FLM_EINVAL
    for k in (-1e-300, -1.0, inf, nan):
        assert _bound(lib, 1.0, 7, 16, k)[0] == FLM_EINVAL, k
    assert _bound(lib, 1.0, 0, 16, 0.0)[0] == 0 and _bound(lib, 1.0, 30, 16, 0.0)[0] == 0
    # a result of 2^63 or more: C 2^f about 2^31.5 and beyond
    assert _bound(lib, 3.0e38, 30, 1, 0.0) == (FLM_ERANGE, 0xDEAD)
    assert _bound(lib, 4.0, 30, 1, 0.0)[0] == FLM_ERANGE and _bound(lib, 2.0, 30, 1, 0.0)[0] == 0   # s^2 = 2^64, 2^62
    assert _bound(lib, 1.0, 0, 1, 1e300)[0] == 0      # the min keeps a huge tail harmless: (s + 1)^2
    assert _bound(lib, 1.0, 0, 2 ** 64 - 1, 1e300)[0] == FLM_ERANGE   # d alone passes 2^63


# ------------------------------------------------------------------ the call's rule
def test_round_check_refusals(lib):
    ok = lambda *a: lib.flm_round_check(*a)
    err = lambda: lib.flm_last_error(None).decode()
    assert ok(4096, 7, 1.0, 4) == 0 and ok(1, 0, 1000.0, 1) == 0 and ok(64 * 4096 + 5, 16, 4.0, 8) == 0
    assert ok(0, 7, 1.0, 4) == FLM_EINVAL
    for a in (0, -1, 9):
        assert ok(4096, 7, 1.0, a) == FLM_EINVAL and "attempts" in err()
    # what flm_codec_check refuses with n = 1, with its code
    for f, c in ((-1, 1.0), (31, 1.0), (7, 0.0), (7, -1.0), (7, float("inf")), (7, float("nan"))):
        assert ok(16, f, c, 1) == FLM_EINVAL == lib.flm_codec_check(f, c, 1), (f, c)
    assert ok(16, 30, 4.0, 1) == FLM_ERANGE == lib.flm_codec_check(30, 4.0, 1)       # B = 2^32 alone has no headroom
    # Q cannot wrap: L B^2 <= 2^64 - 1.  B = 2^30: 15 B^2 fits, 16 B^2 = 2^64 does not
    assert ok(15, 30, 1.0, 1) == 0
    assert ok(16, 30, 1.0, 1) == FLM_ERANGE and "wrap the 64-bit sum" in err()
    # B = 2^14 at the longest row the dither stream has: 2^36 B^2 = 2^64, one above 2^64 - 1; B = 2^13 fits
    assert ok(2 ** 36, 14, 1.0, 1) == FLM_ERANGE and "wrap the 64-bit sum" in err()
    assert ok(2 ** 36, 13, 1.0, 1) == 0
    # L B^2 = 2^64 - 1 exactly is square-free, so only B = 1 reaches it: the wrap rule lets it by (the text is the
    # next rule's, the dither stream's block counter), and one more B^2 is refused by the wrap rule itself
    assert ok(2 ** 64 - 1, 0, 1.0, 1) == FLM_ERANGE and "2^32 blocks" in err()
    assert ok(2 ** 63, 1, 1.0, 1) == FLM_ERANGE and "wrap the 64-bit sum" in err()  # L B^2 = 2^65
    big = 2 ** 31 - 128                                # B = ceil((2 - 2^-23) 2^30), the largest the codec takes
    c_big = float(np.nextafter(np.float32(2.0), np.float32(0.0)))
    assert math.ceil(Fraction(c_big) * 2 ** 30) == big and 4 * big * big <= 2 ** 64 - 1 < 5 * big * big
    assert ok(4, 30, c_big, 1) == 0 and ok(5, 30, c_big, 1) == FLM_ERANGE
    # the dither stream's block counter: ceil(L / 16) <= 2^32
    assert ok(2 ** 36, 0, 1.0, 8) == 0
    assert ok(2 ** 36 + 1, 0, 1.0, 8) == FLM_ERANGE and "2^32 blocks" in err()


def test_device_calls_refuse_without_a_context(lib):
    assert lib.flm_round_select_dev(None, None, 0, 1, 1, 7, 1.0, None, 1, 0, None, None, None, None) == FLM_EINVAL
    assert lib.flm_round_select(None, None, 1, 1, 7, 1.0, None, 1, 0, None, None, None) == FLM_EINVAL
    assert b"round_bound" in lib.flm_version()


# ------------------------------------------------------------------ the agents' options
def test_configure_round_bound_refusals():
    from flamingo_amd.abides.flamingo import protocol as param
    try:
        param.configure(L=4001, codec=False)
        assert param.round_bound() is None
        for off in (0, 0.0, False):
            param.configure(round_bound=off)                                   # off needs nothing
        with pytest.raises(ValueError):
            param.configure(round_bound=1.0)                                   # needs the float inputs
        with pytest.raises(ValueError):
            param.configure(codec=(7, 1.0, "nearest"), l2_clip=2.0, round_bound=1.0)    # ... stochastic ones
        with pytest.raises(ValueError):
            param.configure(codec=(7, 1.0, "stochastic"), l2_clip=0, round_bound=1.0)   # ... and the L2 clip
        assert param.round_bound() is None
        for bad in ((-1.0, 4), (float("nan"), 4), (float("inf"), 4), (1.0, 0), (1.0, 9), (1.0, 2.5)):
            with pytest.raises(ValueError):
                param.configure(codec=(7, 1.0, "stochastic"), l2_clip=2.0, round_bound=bad)
        param.configure(codec=(7, 1.0, "stochastic", 2), rotate=5, l2_clip=2.28125, round_bound=1.0)
        assert param.round_bound() == (1.0, 4)                                # ATTEMPTS defaults to 4
        param.configure(round_bound=(0.0, 8))
        assert param.round_bound() == (0.0, 8)                                # a tuple's tail of 0 is a tail
        param.configure(round_bound=0)
        assert param.round_bound() is None
        param.configure(round_bound=(2.0, 1))
        param.configure(l2_clip=0)                                             # what it stands on goes: it goes too
        assert param.round_bound() is None
        param.configure(l2_clip=2.0, round_bound=(2.0, 1))
        param.configure(codec=(7, 1.0, "nearest"))
        assert param.round_bound() is None and param.l2_clip() == 2.0
        param.configure(codec=(7, 1.0, "stochastic"), round_bound=1.0)
        param.configure(codec=False)
        assert param.round_bound() is None
    finally:
        param.configure(codec=False, L=param.P.vector_len)


def test_driver_option():
    from flamingo_amd.abides.config_flamingo import parse, parse_round_bound
    assert parse(["-c", "flamingo"])[1].round_bound is None and parse_round_bound(None) is None
    assert parse(["-c", "flamingo", "--round_bound", "1"])[1].round_bound == "1"
    assert parse_round_bound("1") == (1.0, 4) and parse_round_bound("2.146,8") == (2.146, 8)
    assert parse_round_bound("0") is None and parse_round_bound("") is None
    with pytest.raises(ValueError):
        parse_round_bound("1,2,3")
