"""The P-256 kernels (flamingo_amd/csrc/flm_p256.hip over flm_fe256.h, flm_jac256.h and flm_fe_row.h) where random inputs do not reach:
the acc == Q and acc == -Q branches of the additions, field elements with all-zero / all-one / single-
bit limbs, every compiled ec_mul_kernel<TPB, WPE>, batch sizes around every packing factor, the auto
routing's thresholds, and the per-element flags of bad inputs with exact neighbours.

Inputs and expected values come from tests/ec_cases.py (the big-int oracle, oracle/ec_oracle.py);
tests/test_ec_cases_cpu.py checks their premises and replays the row field's carry loops on them
without a GPU.  Every comparison is == on integers or bytes.
"""
import numpy as np
import pytest

import ec_cases as C
import ec_oracle as E

pytestmark = pytest.mark.gpu

N = E.N


@pytest.fixture(scope="module", params=[(0, 1), (1, 1), (2, 1), (0, 2), (0, 4)],
                ids=["per_lane", "coop", "row", "straus2", "straus4"])
def eng(request):
    """The five engines of tests/test_ec_gpu.py: ec_mul_kernel, ec_mul_coop_kernel, ec_mul_row_kernel and
    ec_mul_straus_kernel<2> / <4> (the combine only; flm_ec_mul keeps one lane per product there)."""
    from flamingo_amd import MaskEngine
    e = MaskEngine(0)
    e.set_tuning("ec_coop", request.param[0])
    e.set_tuning("ec_terms", request.param[1])
    yield e
    e.close()


@pytest.fixture(scope="module")
def lane_eng():
    from flamingo_amd import MaskEngine
    e = MaskEngine(0)
    e.set_tuning("ec_coop", 0)
    yield e
    e.close()


def _wire(points):
    return np.frombuffer(b"".join(E.wire(pt) for pt in points), np.uint8).reshape(-1, 64).copy()


def _combine_all(eng, c1, shares, lam, want):
    """ec_combine with and without c1, negate on and off, against want[(with_c1, negate)]."""
    for with_c1 in (True, False):
        for neg in (True, False):
            assert eng.ec_combine(c1 if with_c1 else None, shares, lam, negate=neg) == want[(with_c1, neg)], \
                (with_c1, neg)


# ------------------------------------------------------------------ 1. exceptional scalars
def test_exceptional_scalars(eng):
    """k = n + 30 ends on acc == Q (the doubling branch of the addition), k = n on acc == -Q."""
    pts, ks, want = C.exceptional_cases()
    got = eng.ec_mul(pts, ks)
    assert got == want
    for pt, k, g in zip(pts, ks, got):
        if k == N:
            assert g is None
        if k == N + 30:
            assert g == C.mulc(30, pt) and g is not None


# ------------------------------------------------------------------ 2. structured limbs
@pytest.mark.parametrize("family", ["normal", "mont"])
def test_structured_points(eng, family):
    """Abscissas with limbs 0, 0xffffffff and single bits, in the row kernel's normal form and in the
    other kernels' Montgomery form; scalars 1, 2, 3 and 15 return the table entries themselves."""
    pts, ks, want = C.structured_cases(family)
    assert eng.ec_mul(pts, ks) == want


@pytest.mark.parametrize("family", ["normal", "mont"])
def test_structured_points_combine(eng, family):
    """The same points as the shares (and c1) of a T = 4 combine: the Straus kernels' tables and the
    finish kernel's additions and inversion see them too."""
    c1, shares, lam = C.structured_combine(family)
    assert eng.ec_combine(c1, shares, lam) == C.combine_expect(c1, shares, lam, True)
    assert eng.ec_combine(None, shares, lam, negate=False) == C.combine_expect(None, shares, lam, False)


# ------------------------------------------------------------------ 3. batch edges
@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 63, 64, 65, 127, 128, 129, 255, 256, 257])
def test_batch_edges(eng, n):
    p = C.pool(n)
    assert eng.ec_mul(p.points, p.scalars) == p.products


# ------------------------------------------------------------------ 4. every per-lane instantiation
@pytest.mark.parametrize("waves", [1, 4, 8])
@pytest.mark.parametrize("threads", [64, 128, 256])
def test_every_per_lane_instantiation(lane_eng, threads, waves):
    """ec_mul_kernel<TPB, WPE> for every (ec_threads, ec_waves): the 4 and 8 budgets spill to scratch."""
    p = C.pool()
    T, D = C.INSTANCE_SHAPE
    c1, shares, lam = C.combine_case(T, D)
    lane_eng.set_tuning("ec_threads", threads)
    lane_eng.set_tuning("ec_waves", waves)
    try:
        assert lane_eng.ec_mul(p.points, p.scalars) == p.products
        assert lane_eng.ec_combine(c1, shares, lam) == C.combine_variants(T, D)[(True, True)]
    finally:
        lane_eng.set_tuning("ec_threads", 64)
        lane_eng.set_tuning("ec_waves", 1)


# ------------------------------------------------------------------ 5. combine shapes
@pytest.mark.parametrize("T,D", C.COMBINE_SHAPES)
def test_combine_shapes(eng, T, D):
    """A workgroup spanning two terms, partial Straus groups, the finish kernel's 8-lane split at
    T < 8, = 8, > 8 and its 8 elements per workgroup at D = 7, 8, 9."""
    c1, shares, lam = C.combine_case(T, D)
    _combine_all(eng, c1, shares, lam, C.combine_variants(T, D))


# ------------------------------------------------------------------ 6. exceptional combines
@pytest.mark.parametrize("k", range(17))
def test_exceptional_combines(eng, k):
    """Equal and opposite terms in columns 0, 5 and 11 of a D = 12 batch of ordinary columns; lambda 0, n
    and n + 30 (the last ends every product of its term on acc == Q inside the scalar multiplication)."""
    case = C.exceptional_combines()[k]
    pts, seeds = eng.ec_combine(case.c1, case.shares, case.lambdas)
    assert pts == case.want_points, case.name
    assert seeds == case.want_seeds, case.name
    if case.name.startswith(("opposite_", "c1_equals_sum")):
        for i in case.special:
            if case.c1 is None or case.name.startswith("c1_equals_sum"):
                assert pts[i] is None and seeds[i] == C.ZERO_SEED
            else:
                assert pts[i] == case.c1[i]


# ------------------------------------------------------------------ 7. flags
def test_ec_mul_flags_are_per_element(eng):
    """flm_ec_mul over the C ABI fills out and flags_out before it returns FLM_EINVAL: bit 1 exactly at
    the bad elements (x = p and x = 5 + p are congruent to valid abscissas: only the range check can
    tell), and every neighbour's product exact."""
    from flamingo_amd._lib import p_u32, p_u8
    wires, ks, want = C.flag_mul_case()
    pw = np.frombuffer(b"".join(wires), np.uint8).reshape(-1, 64).copy()
    sw = np.frombuffer(b"".join(k.to_bytes(32, "big") for k in ks), np.uint8).reshape(-1, 32).copy()
    out = np.full((C.FLAG_N, 64), 0xAA, np.uint8)
    fl = np.full(C.FLAG_N, 0xFFFFFFFF, np.uint32)
    rc = eng.lib.flm_ec_mul(eng.ctx, p_u8(pw), p_u8(sw), C.FLAG_N, p_u8(out), p_u32(fl))
    assert rc != 0 and b"element 0: input is not a point on P-256" in eng.lib.flm_last_error(eng.ctx)
    assert [i for i in range(C.FLAG_N) if fl[i] & 2] == sorted(C.MUL_BAD)
    for i in range(C.FLAG_N):
        if i not in C.MUL_BAD:
            assert int(fl[i]) == 0 and bytes(out[i]) == E.wire(want[i]), i
    # 64 zero bytes are what comes back for infinity, but as an input they are not a point
    # (include/flamingo_hip.h: each coordinate of an input is on the curve): flagged like the rest
    assert C.MUL_BAD[6] == "zero_wire" and fl[6] & 2
    with pytest.raises(RuntimeError, match="not a point on P-256"):
        eng.ec_mul_wire(np.zeros((1, 64), np.uint8), sw[:1])


def test_ec_combine_dev_flags_are_per_element(eng):
    """flm_ec_combine_dev writes the flags and does not check them: bit 0 exactly where c1 is bad, bit 1
    exactly where a share is bad, and the columns in between exact."""
    import torch
    c1_w, sh_w, lam, good, want_pts, want_seeds = C.flag_combine_case()
    dev = torch.device("cuda:0")
    D, T = C.FLAG_N, C.COMBINE_T
    c1_t = torch.from_numpy(np.frombuffer(b"".join(c1_w), np.uint8).reshape(D, 64).copy()).to(dev)
    sh_t = torch.from_numpy(np.frombuffer(b"".join(b"".join(r) for r in sh_w), np.uint8).reshape(T, D, 64).copy()).to(dev)
    lam_t = torch.from_numpy(np.frombuffer(b"".join(k.to_bytes(32, "big") for k in lam), np.uint8)
                             .reshape(T, 32).copy()).to(dev)
    seeds_t = torch.zeros((D, 32), dtype=torch.uint8, device=dev)
    pts_t = torch.zeros((D, 64), dtype=torch.uint8, device=dev)
    flags_t = torch.full((D,), -1, dtype=torch.int32, device=dev)
    eng.ec_combine_dev(c1_t, sh_t, lam_t, seeds_t, flags_t, points_out=pts_t)
    torch.cuda.synchronize()
    fl = flags_t.cpu().numpy().view(np.uint32)
    assert [i for i in range(D) if fl[i] & 1] == sorted(C.C1_BAD)
    assert [i for i in range(D) if fl[i] & 2] == sorted({c for _, c in C.SHARE_BAD})
    pts, seeds = pts_t.cpu().numpy(), seeds_t.cpu().numpy()
    assert good == [2, 5, 7]
    for i in good:
        assert int(fl[i]) == 0 and bytes(pts[i]) == E.wire(want_pts[i]) and bytes(seeds[i]) == want_seeds[i], i
    # a bad share counts as infinity and a bad c1 too; the rest of the column's sum is still exact
    c1, shares, lam_ = C.combine_case(T, D)
    i = 3                                                      # share (1, 3) is bad, c1 and the other terms are not
    rest = E.add(c1[i], E.neg(E.add(C.mulc(lam_[0], shares[0][i]), C.mulc(lam_[2], shares[2][i]))))
    assert bytes(pts[i]) == E.wire(rest)


# ------------------------------------------------------------------ 8. auto routing
def test_auto_routing_thresholds():
    """ec_coop = -1 (the default every agent uses): the row kernel up to 20 products per CU, the
    cooperative kernel up to 128 per CU, one lane per product beyond; the same products on either side
    of each threshold."""
    from flamingo_amd import MaskEngine
    p = C.pool()
    pw = _wire(p.points)
    sw = np.frombuffer(b"".join(k.to_bytes(32, "big") for k in p.scalars), np.uint8).reshape(-1, 32)
    ww = _wire(p.products)
    with MaskEngine(0) as e:
        assert e.get_tuning("ec_coop") == -1
        c = e.cu_count()
        for n in (20 * c, 20 * c + 1, 128 * c, 128 * c + 1):
            reps = -(-n // 257)
            out, fl = e.ec_mul_wire(np.tile(pw, (reps, 1))[:n], np.tile(sw, (reps, 1))[:n])
            assert not fl.any(), n
            assert np.array_equal(out, np.tile(ww, (reps, 1))[:n]), n
