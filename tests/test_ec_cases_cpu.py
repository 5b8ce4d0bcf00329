"""The premises of tests/test_ec_edges_gpu.py, checked without a GPU: the edge inputs of
tests/ec_cases.py are what they claim to be, and the row field's carry loops end on every one of
them before any of them reaches a GPU.

The row kernel (ec_mul_row_kernel, flm_fe_row.h) normalises with `do { ... } while (__any(c != 0))`
passes, so an input on which a loop did not end would hang a wave.  replay() below restates that
kernel's own sequence of field operations -- the on-curve check, coop_dbl_w, coop_add_w with its
level-6 selection, RowField::dbl (dbl-2001-b) on the acc == Q path, add-2007-bl everywhere else, the
conversion to Montgomery form -- over the Python model of the row field (tools/ec_row_model.py:
row_mul, row_add, row_sub) and counts the passes of every loop.  MAX_PASSES is a condition on the
inputs, not a measurement: an input that exceeds it is not sent to the GPU.

Observed maxima over everything replayed here (table builds of all normal-form structured points,
full chains of eight points by n + 30, n, 2^256 - 1 and a random scalar, the discarded additions of
a row whose digit is zero, the range / on-curve check of the bad inputs):
    product columns 7, NIST fold 6, add 5, sub 11, canon 8.
This replay is also what first showed RowField::dbl computing Y3 with 4 gamma^2 for 8 gamma^2 (the
n + 30 chain came out with a wrong y, the value the GPU then returned): DESIGN.md section 5.
"""
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))

import ec_cases as C  # noqa: E402
import ec_oracle as E  # noqa: E402
import ec_row_model as M  # noqa: E402

MAX_PASSES = 32
P, N = E.P, E.N


# ------------------------------------------------------------------ the case lists
def test_structured_points_are_on_the_curve():
    S = C.structured_points()
    for family in ("normal", "mont"):
        pts = S[family]
        assert len(pts) >= 30 and len(set(pts)) == len(pts)
        assert all(E.on_curve(pt) and 0 <= pt[0] < P and 0 <= pt[1] < P for pt in pts)
        assert sum(1 for x, y in pts if (x, P - y) in pts) == 8          # four of them with both signs
    cand = set(C.limb_candidates())
    assert all(x in cand for x, _ in S["normal"])
    assert all(x * C.R % P in cand for x, _ in S["mont"])                # the Montgomery limbs are the candidate's
    xs = {x for x, _ in S["normal"]}
    assert {0, 5, 6, 8, 9, P - 3, 2**32, 2**32 - 1, 2**128 - 1, P - 2**32} <= xs


def test_pool_is_distinct_and_matches_the_oracle():
    p = C.pool()
    assert len(p.points) == len(set(p.points)) == 257 and len(set(p.scalars)) == 257
    assert all(E.on_curve(pt) for pt in p.points)
    assert C.pool(5).points == p.points[:5] and C.pool(5).products == p.products[:5]
    for i in (0, 100, 256):
        assert p.products[i] == E.mul(p.scalars[i], p.points[i])


def test_naf5_recodes_the_scalar():
    for k in [0, 1, 15, 16, 17, 31, N, N + 30, 2**255, 2**256 - 1, C.RANDOM_SCALAR] + C.pool(20).scalars:
        d = C.naf5(k)
        assert len(d) == C.NAF_LEN and sum(v << i for i, v in enumerate(d)) == k
        assert all(v == 0 or (v & 1 and -15 <= v <= 15) for v in d)
        assert all(not any(d[i + 1:i + 5]) for i, v in enumerate(d) if v)


def test_chain_events_of_the_exceptional_scalars():
    assert C.chain_events(N + 30) == [(0, 15, "double")]
    assert C.chain_events(N) == [(0, -15, "infinity")]
    for k in (N + 1, N - 1, 2**256 - 1, N + 15, N + 31, 15, 16, 30, 31, 32, 33, 2**255):
        assert C.chain_events(k) == []


def test_only_the_listed_scalars_meet_an_exceptional_addition():
    for k in set(C.gpu_scalars()):
        kinds = [kind for _, _, kind in C.chain_events(k)]
        assert kinds == ([C.EVENTS[k]] if k in C.EVENTS else []), hex(k)
    assert set(C.EVENTS) <= set(C.EXC_SCALARS)


def test_the_window_around_n_has_two_exceptional_scalars():
    hits = {k - N: C.chain_events(k) for k in range(N - 200, N + 201) if C.chain_events(k)}
    assert hits == {0: [(0, -15, "infinity")], 30: [(0, 15, "double")]}


def test_combine_expect_is_the_oracle_combine():
    c1, shares, lam = C.combine_case(3, 5)
    for with_c1 in (True, False):
        for neg in (True, False):
            assert C.combine_variants(3, 5)[(with_c1, neg)] == E.combine(c1 if with_c1 else None, shares, lam, neg)


def test_exceptional_combines_are_exceptional():
    cases = {c.name: c for c in C.exceptional_combines()}
    assert len(cases) == 17
    a = C.EXC_A
    for c in cases.values():
        assert len(c.want_points) == C.EXC_D and all(E.on_curve(pt) for pt in c.want_points)
        ordinary = [i for i in range(C.EXC_D) if i not in c.special]
        assert all(c.want_points[i] is not None for i in ordinary)
    for i in C.EXC_SPECIAL:
        c = cases["equal_shares_unit-none"]
        assert c.shares[0][i] == c.shares[1][i] and c.want_points[i] == E.neg(E.mul(2, c.shares[0][i]))
        c = cases["equal_products-none"]
        assert E.mul(2 * a, c.shares[0][i]) == E.mul(a, c.shares[1][i]) and c.shares[0][i] != c.shares[1][i]
        # the Straus lane meets it as acc == Q: after the top digit of 2a the accumulator is d P, doubled
        # once it equals the top digit of a times 2P
        assert C.naf5(2 * a)[1:] == C.naf5(a)[:-1]
        for name in ("opposite_products", "opposite_unit"):
            assert cases[name + "-none"].want_points[i] is None
            assert cases[name + "-none"].want_seeds[i] == C.ZERO_SEED
            assert cases[name + "-c1"].want_points[i] == cases[name + "-c1"].c1[i]
        assert cases["c1_equals_sum-c1"].want_points[i] is None
        for name in ("c1_equals_minus_sum-c1", "c1_doubles_in_finish-c1"):
            assert cases[name].want_points[i] == E.mul(2, cases[name].c1[i])
    c = cases["lambda_n_plus_30-none"]
    assert c.want_points == [E.neg(E.add(E.mul(30, p0), E.mul(c.lambdas[1], p1))) for p0, p1 in zip(*c.shares)]
    for name in ("lambda_zero", "lambda_n"):
        c = cases[name + "-none"]
        assert c.want_points == [E.neg(E.mul(c.lambdas[1], pt)) for pt in c.shares[1]]


def test_bad_inputs_are_bad_and_two_are_congruent_to_points():
    bad = C.bad_wire_points()
    dec = {k: (int.from_bytes(v[:32], "big"), int.from_bytes(v[32:], "big")) for k, v in bad.items()}
    for name, (x, y) in dec.items():
        assert not (x < P and y < P and E.on_curve((x, y))), name
    for name in ("x_p", "x_5_plus_p"):
        x, y = dec[name]
        assert x >= P and E.on_curve((x % P, y))        # only the range check rejects these
    assert dec["x_5_plus_p"][0] == 5 + P and dec["x_all_ones"][0] == 2**256 - 1
    wires, ks, want = C.flag_mul_case()
    assert [i for i, w in enumerate(want) if w is None] == sorted(C.MUL_BAD)
    assert C.flag_combine_case()[3] == [2, 5, 7]


# ------------------------------------------------------------------ the row kernel, replayed
class RowField:
    """RowField of flm_p256.hip over the Python model; records the most passes any loop took."""

    def __init__(self):
        self.peak = {"mul_columns": 0, "mul_fold": 0, "add": 0, "sub": 0, "canon": 0}

    def _seen(self, **kw):
        for k, v in kw.items():
            assert v <= MAX_PASSES, (k, v)
            self.peak[k] = max(self.peak[k], v)

    def mul(self, a, b):
        r, p1, p2 = M.row_mul(a, b)
        self._seen(mul_columns=p1, mul_fold=p2)
        return r

    def sqr(self, a):
        return self.mul(a, a)

    def add(self, a, b):
        r, p = M.row_add(a, b)
        self._seen(add=p)
        return r

    def sub(self, a, b):
        r, p = M.row_sub(a, b)
        self._seen(sub=p)
        return r

    def neg(self, a):
        return self.sub(0, a)

    @staticmethod
    def is_zero(a):
        return a == 0 or a == P

    def canon(self, a):
        """row::canon: a - p with the borrows passed along the row; a itself when the top borrows."""
        d = [x - y for x, y in zip(M.limbs(a), M.limbs(P))]
        c, lo = [x >> 32 for x in d], [x & M.M32 for x in d]
        top = passes = 0
        while True:
            top += c[7]
            d = [lo[r] + (c[r - 1] if r else 0) for r in range(8)]
            c, lo = [x >> 32 for x in d], [x & M.M32 for x in d]
            passes += 1
            assert passes <= MAX_PASSES
            if not any(c):
                break
        self._seen(canon=passes)
        out = M.val(lo) if top == 0 else a
        assert out == a % P
        return out

    def dbl(self, X, Y, Z):
        """RowField::dbl, dbl-2001-b."""
        delta, gamma = self.sqr(Z), self.sqr(Y)
        beta = self.mul(X, gamma)
        t = self.mul(self.sub(X, delta), self.add(X, delta))
        alpha = self.add(self.add(t, t), t)
        beta4 = self.add(self.add(beta, beta), self.add(beta, beta))
        X3 = self.sub(self.sqr(alpha), self.add(beta4, beta4))
        Z3 = self.sub(self.sub(self.sqr(self.add(Y, Z)), gamma), delta)
        g2 = self.sqr(gamma)
        g4 = self.add(g2, g2)
        g8 = self.add(g4, g4)
        g8 = self.add(g8, g8)
        return X3, self.sub(self.mul(alpha, self.sub(beta4, X3)), g8), Z3


def load_check(f, x, y):
    """The range and on-curve test at the top of ec_mul_row_kernel."""
    rhs = f.add(f.sub(f.mul(f.sqr(x), x), f.add(f.add(x, x), x)), E.B)
    in_x, in_y = f.canon(x) == x, f.canon(y) == y
    on_c = f.canon(f.sqr(y)) == f.canon(rhs)          # all three run whatever the others say
    return in_x and in_y and on_c


def coop_dbl_w(f, acc):
    X, Y, Z, W = acc
    t = f.sub(f.sqr(X), W)
    alpha = f.add(f.add(t, t), t)
    a2 = f.sqr(alpha)
    beta = f.mul(X, f.sqr(Y))
    b2 = f.add(beta, beta)
    b4 = f.add(b2, b2)
    b8 = f.add(b4, b4)
    g = f.sqr(f.sqr(Y))
    g = f.add(g, g)
    g = f.add(g, g)
    g8 = f.add(g, g)
    yz = f.mul(Y, Z)
    z3 = f.add(yz, yz)
    x3 = f.sub(a2, b8)
    y3 = f.sub(f.mul(alpha, f.sub(b4, x3)), g8)
    return x3, y3, z3, f.mul(f.add(g8, g8), W)


def coop_add_w(f, acc, Q, neg, sel=True):
    """Every level runs whatever the operands are (the waves cannot branch around the votes of the
    carry loops); level 6 then picks the ordinary result or an exceptional one."""
    X1, Y1, Z1, W1 = acc
    X2, Y2, Z2 = Q
    if neg:
        Y2 = f.neg(Y2)
    z1z1, z2z2 = f.sqr(Z1), f.sqr(Z2)
    zz = f.sqr(f.add(Z1, Z2))
    s1a = f.mul(Y1, Z2)
    u2, u1 = f.mul(X2, z1z1), f.mul(X1, z2z2)
    z3p = f.sub(f.sub(zz, z1z1), z2z2)
    s2a = f.mul(Y2, Z1)
    s1 = f.mul(s1a, z2z2)
    h = f.sub(u2, u1)
    i = f.sqr(f.add(h, h))
    s2 = f.mul(s2a, z1z1)
    z3 = f.mul(z3p, f.sub(u2, u1))
    j = f.mul(h, i)
    v = f.mul(u1, i)
    v2 = f.add(v, v)
    r = f.sub(s2, s1)
    r = f.add(r, r)
    rr = f.sqr(r)
    w3 = f.sqr(f.sqr(z3))
    x3 = f.sub(f.sub(rr, j), v2)
    y3a = f.mul(r, f.sub(v, x3))
    s1j = f.mul(s1, j)
    s1j2 = f.add(s1j, s1j)
    R = (x3, f.sub(y3a, s1j2), z3, w3)
    if f.is_zero(Z1):
        R = (X2, Y2, Z2, f.sqr(f.sqr(Z2)))
    elif f.is_zero(Z2):
        R = acc
    elif f.is_zero(h):
        d = f.dbl(X1, Y1, Z1) if f.is_zero(r) else (1, 1, 0)
        R = d + (f.sqr(f.sqr(d[2])),)
    return R if sel else acc


def affine(X, Y, Z):
    if Z % P == 0:
        return None
    zi = pow(Z, -1, P)
    return (X * zi * zi % P, Y * zi * zi * zi % P)


def build_table(f, pt):
    PW = (pt[0], pt[1], 1, 1) if pt is not None else (1, 1, 0, 0)     # an invalid point goes in as infinity
    P2 = coop_dbl_w(f, PW)[:3]
    tab, t = [PW[:3]], PW
    for _ in range(7):
        t = coop_add_w(f, t, P2, False)
        tab.append(t[:3])
    return tab


def replay(f, pt, k, shadow=False):
    """ec_mul_row_kernel for one row; shadow also runs the additions a row computes and discards while
    its own digit is zero and another row of the wave has one (table entry 0)."""
    assert load_check(f, *pt)
    tab = build_table(f, pt)
    dig = C.naf5(k)
    acc = (1, 1, 0, 0)
    for w in range(C.NAF_LEN - 1, -1, -1):
        acc = coop_dbl_w(f, acc)
        v = dig[w]
        if v:
            acc = coop_add_w(f, acc, tab[abs(v) >> 1], v < 0)
        elif shadow:
            acc = coop_add_w(f, acc, tab[0], False, sel=False)
    rm = C.R % P
    X, Y, Z = (f.canon(f.mul(c, rm)) for c in acc[:3])
    return affine(X * C.R_INV % P, Y * C.R_INV % P, Z * C.R_INV % P)


@pytest.fixture(scope="module")
def field():
    f = RowField()
    yield f
    print("\nrow model, most passes per loop:", f.peak)


def test_row_replay_table_build_of_every_structured_point(field):
    for pt in C.structured_points()["normal"]:
        assert load_check(field, *pt)
        tab = build_table(field, pt)
        assert [affine(*e) for e in tab] == [C.mulc(2 * t + 1, pt) for t in range(8)]


REPLAY_POINTS = [0, 3, 9, 20, 33, 47, 55, -1]      # indices into the normal-form family
REPLAY_SCALARS = [N + 30, N, 2**256 - 1, C.RANDOM_SCALAR]


@pytest.mark.parametrize("idx", REPLAY_POINTS)
def test_row_replay_full_chain(field, idx):
    pt = C.structured_points()["normal"][idx]
    for n, k in enumerate(REPLAY_SCALARS):
        assert replay(field, pt, k, shadow=(k == N + 30 and idx in (0, -1))) == C.mulc(k, pt), hex(k)


def test_row_replay_range_check_of_the_bad_inputs(field):
    for name, w in C.bad_wire_points().items():
        x, y = int.from_bytes(w[:32], "big"), int.from_bytes(w[32:], "big")
        assert not load_check(field, x, y), name
    # an invalid point enters the chain as infinity (1, 1, 0): the whole chain on it stays there
    acc = (1, 1, 0, 0)
    inf_tab = build_table(field, None)
    for v in C.naf5(C.RANDOM_SCALAR)[::-1][:40]:
        acc = coop_dbl_w(field, acc)
        if v:
            acc = coop_add_w(field, acc, inf_tab[abs(v) >> 1], v < 0)
        assert acc[2] % P == 0


def test_row_replay_peak_is_under_the_cap(field):
    """Runs last in this module: the maxima of everything replayed above (recorded in the docstring)."""
    assert max(field.peak.values()) <= MAX_PASSES
    assert field.peak["sub"] > 1 and field.peak["mul_columns"] > 1         # the edge inputs do carry further
