"""Premises of tests/fe_cases.py, without a GPU: the integer models of flm_fe256.h's lane and scalar
layers agree with Python's own modular arithmetic, every directed operand lands where its list says
by the model (window position, fe_sqr event, carry count, row pass count), every target or event
listed as unreachable is asserted so, and the random lists alone reach none of the reduction window
nor the `x + c` carry of fe_sqr -- so the directed cases are what covers them.
tests/test_fe_ops_gpu.py runs the same lists through the device code."""
import fe_cases as F

P, N, R = F.P, F.N, F.R
R_INV = {m: pow(R, -1, m) for m in (P, N)}


# ------------------------------------------------------------------ the models against big integers
def test_models_agree_with_big_integers_on_the_random_pairs():
    for a, b in F.random_pairs(P):
        t, counts = F.mul_columns(a, b)
        assert F.val(t) == a * b and all(0 <= c <= mx for c, mx in zip(counts, F.MUL_MAX_COUNT))
        assert F.fe_mul_model(a, b) == a * b * R_INV[P] % P
        t, _ = F.sqr_columns(a)
        assert F.val(t) == a * a
        assert F.fe_sqr_model(a) == a * a * R_INV[P] % P
    for a, b in F.random_pairs(N):
        T, t8 = F.sc_mul_T(a, b)
        assert (T + t8 * R) * R == a * b + (-a * b * pow(N, -1, R) % R) * N
        assert F.sc_mul_model(a, b) == a * b * R_INV[N] % N


def test_models_agree_on_the_structured_pairs():
    for m in (P, N):
        s = F.structured_values(m)
        assert 30 <= len(s) <= 45 and len(set(s)) == len(s) and all(0 <= v < m for v in s)
        for v in (0, 1, 2, m - 1, m - 2, (m - 1) // 2, (m + 1) // 2, R - 2**224 - 1, R % m, R * R % m, m - R % m):
            assert v in s
        pairs = F.structured_pairs(m)
        assert len(pairs) == len(s) ** 2 + F.N_RANDOM
        for a, b in pairs[:len(s) ** 2]:
            T = F.mul_T(a, b, m)
            assert T < 2 * m and F.reduce_once(T % R, T >> 256, m) == a * b * R_INV[m] % m
    for a in F.structured_values(P):
        assert F.fe_sqr_model(a) == a * a * R_INV[P] % P


def test_random_lists_alone_miss_the_window_and_the_addc_carry():
    """what the directed cases are for: 2,000 random products per modulus never put T in [m, 2^256),
    and 2,000 random squarings never take `xh += (n < x)`"""
    for m in (P, N):
        assert not any(F.in_window(F.mul_T(a, b, m), m) for a, b in F.random_pairs(m))
        assert not any(F.in_window(F.mul_T(a, R * R % m, m), m) for a, _ in F.random_pairs(m))
    assert not any(F.in_window(F.fe_sqr_T(a), P) for a, _ in F.random_pairs(P))
    assert not any("addc" in ev for a, _ in F.random_pairs(P) for ev in F.sqr_columns(a)[1])


# ------------------------------------------------------------------ fe_mul's carry counts
def test_mul_count_cases_reach_the_largest_count_and_zero_in_every_column():
    cases = F.mul_count_cases()
    assert [(K, kind) for K, kind, *_ in cases] == [(K, kind) for K in range(15) for kind in ("max", "zero")]
    assert F.MUL_MAX_COUNT == [0, 1, 2, 3, 4, 5, 6, 7, 6, 5, 4, 3, 2, 1, 0]
    for K, kind, a, b, count in cases:
        assert 0 < a < P and 0 < b < P
        assert F.mul_columns(a, b)[1][K] == count == (F.MUL_MAX_COUNT[K] if kind == "max" else 0)


# ------------------------------------------------------------------ the reduction window
def test_window_targets():
    for m in (P, N):
        t = F.window_targets(m)
        assert t[:5] == (m + 1, m + 2**32, R - 1, R, R + 1) and len(t) == 21
        assert all(m + 1 <= T < R for T in t[5:]) and all(T < 2 * m for T in t)


def test_mul_window_cases_hit_every_target():
    for m in (P, N):
        cases = F.mul_window_cases(m)
        assert [T for _, T, _, _ in cases] == list(F.window_targets(m))
        for name, T, a, b in cases:
            assert 0 < a < m and 0 < b < m
            assert F.mul_T(a, b, m) == T, name
            assert F.reduce_once(T % R, T >> 256, m) == T - m == a * b * R_INV[m] % m
        # a selection on t8 alone returns T, not T - m, exactly at the targets below 2^256
        assert sum(1 for _, T, _, _ in cases if F.in_window(T, m)) == 19


def test_to_mont_window_cases_and_their_unreachable_targets():
    assert F.to_mont_unsolved(P) == ("2^256-1", "2^256", "p+0xcfbcfbf92a865bdaa7c476e49ff038dda1b45c963484e1a5fbc54180")
    assert F.to_mont_unsolved(N) == ("2^256",)
    for m in (P, N):
        b = R * R % m
        for name, T, a in F.to_mont_window_cases(m):
            if a is not None:
                assert 0 < a < m and F.mul_T(a, b, m) == T, name
            else:
                # no M = T 2^256 m^-1 (mod b) below 2^256 gives 0 <= a < m: try every M of that class
                # from below T 2^256 / m - b (where a >= m) up to 2^256
                r = T * R * pow(m, -1, b) % b
                M = r + (T * R // m - 2 * b - r) // b * b
                assert (T * R - M * m) // b >= m
                while M < R:
                    assert M < 0 or not 0 <= (T * R - M * m) // b < m, name
                    M += b
        assert sum(1 for _, T, a in F.to_mont_window_cases(m) if a is not None and F.in_window(T, m)) >= 16


def test_from_mont_never_reaches_the_window():
    """b = 1: the solver has no solution for any target, and no listed value gets there"""
    assert F.FROM_MONT_REACHABLE == ()
    assert all(F.solve_window(T, 1, P) is None for T in F.window_targets(P))
    assert all(F.fe_mul_T(a, 1) == a * R_INV[P] % P for a in F.from_mont_values() + (P - 1, P - 2))


def test_sqr_window_cases():
    cases = F.sqr_window_cases()
    assert F.sqr_unsolved() == ("2^256-1",)
    solved = [(name, T, a) for name, T, a in cases if a is not None]
    assert len(solved) == F.SQR_WINDOW_SMALL + 4
    for name, T, a in solved:
        assert 0 < a < P and F.fe_sqr_T(a) == T and a * a * R_INV[P] % P == T - P, name
    assert sum(1 for _, T, _ in solved if F.in_window(T, P)) == F.SQR_WINDOW_SMALL + 2
    # the unsolved target is not a square at all: (T - p) 2^256 has no root
    assert F.sqrt_p((R - 1 - P) * R % P) is None


def test_sc_mul_unreduced_first_operand():
    """a = n gives T = n exactly (the one way to the window's lower end) and the result 0; a = 2^256 - 1
    and n + 1 stay below 2n"""
    for a, b in F.sc_mul_unreduced_cases():
        T, t8 = F.sc_mul_T(a, b)
        assert T + t8 * R < 2 * N
        assert F.sc_mul_model(a, b) == a * b * R_INV[N] % N
        if a == N:
            assert (T, t8) == (N, 0)
    assert {a for a, _ in F.sc_mul_unreduced_cases()} == {N, R - 1, N + 1}


# ------------------------------------------------------------------ fe_sqr's events
def test_sqr_event_cases_cover_every_reachable_event():
    cases = F.sqr_event_cases()
    got = {(K, e) for K, e, _ in cases}
    want = {(K, e) for K in range(15) for e in F.SQR_EVENTS + ("none",) if (K, e) not in F.SQR_UNREACHABLE}
    assert got == want and len(cases) == len(want) == 47
    for K, e, a in cases:
        ev = F.sqr_columns(a)[1][K]
        assert 0 < a < P and (not ev if e == "none" else e in ev), (K, e, hex(a))
        assert F.fe_sqr_model(a) == a * a * R_INV[P] % P
    # the issue's witness takes the x + c carry in column 1
    assert "addc" in F.sqr_columns(0x80000001FFFFFFFE)[1][1]


def test_sqr_unreachable_events_are_unreachable():
    """columns 0 and 14 take no event and odd columns no "diag", on every input of every list"""
    assert sorted(F.SQR_UNREACHABLE) == sorted([(0, e) for e in F.SQR_EVENTS] + [(14, e) for e in F.SQR_EVENTS] +
                                               [(K, "diag") for K in range(1, 14, 2)])
    inputs = [a for _, _, a in F.sqr_event_cases()] + list(F.unary_values(P)) + \
             [a for _, _, a in F.sqr_window_cases() if a is not None] + [P - 1, R - 1, R - 2**224 - 1]
    for a in inputs:
        ev = F.sqr_columns(a)[1]
        assert not any(e in ev[K] for K, e in F.SQR_UNREACHABLE), hex(a)


# ------------------------------------------------------------------ add and subtract
def test_add_and_sub_edge_cases():
    for m in (P, N):
        sums = {a + b for a, b in F.add_edge_cases(m)}
        assert sums == {m - 1, m, m + 1, R - 1, R, R + 1}
        assert all(0 <= a < m and 0 <= b < m for a, b in F.add_edge_cases(m))
        subs = F.sub_edge_cases(m)
        assert any(a == b for a, b in subs) and any(a == b - 1 for a, b in subs)
        assert any(a == 0 and b for a, b in subs) and any(b == 0 and a for a, b in subs)


def test_range_values_straddle_the_modulus():
    for m in (P, N):
        v = F.range_values(m)
        assert {m - 1, m, m + 1, R - 1, 0} <= set(v) and all(0 <= x < R for x in v)


# ------------------------------------------------------------------ the row layer
def test_row_model_canon_and_is_zero():
    for a in F.row_search_values() + F.row_values("canon"):
        c, passes = F.RM.row_canon(a)
        assert c == a % P and passes >= 1, hex(a)
        assert F.RM.row_is_zero(a) == (a % P == 0)
    assert [F.RM.row_canon(a)[0] for a in (0, P - 1, P, P + 1, R - 1)] == [0, P - 1, 0, 1, R - 1 - P]
    assert [F.RM.row_is_zero(a) for a in (0, P, 1, P - 1, 2 * P - R)] == [True, True, False, False, False]


def test_row_pass_search_reaches_the_recorded_counts():
    found = F.row_pass_search()
    assert F.row_max_passes() == F.ROW_MAX_PASSES
    assert F.ROW_MAX_PASSES == {("mul", "columns"): 7, ("mul", "fold"): 11, ("add", "fold"): 11, ("sub", "fold"): 11,
                                ("canon", "borrow"): 8}
    counts = {}
    for (op, which, n), (a, b) in found.items():
        counts.setdefault((op, which), set()).add(n)
        got = F.row_passes(op, a, b)
        assert got[{"columns": 0, "fold": len(got) - 1, "borrow": 0}[which]] == n
    assert counts[("mul", "columns")] == set(range(8)) and counts[("mul", "fold")] == set(range(12))
    assert counts[("add", "fold")] == counts[("sub", "fold")] == set(range(12))
    assert counts[("canon", "borrow")] == {1, 2, 3, 4, 5, 7, 8}
    # far above what random operands take
    assert max(max(F.row_passes("mul", a, b)) for a, b in F.row_pairs("mul")[-600:]) <= 3


def test_row_lists_results_are_the_residues():
    for op in ("mul", "add", "sub"):
        pairs = F.row_pairs(op)
        assert len(pairs) < 4000
        for a, b in pairs:
            r = F.row_expect(op, a, b)
            assert 0 <= r < R and r % P == F.row_residue(op, a, b), (op, hex(a), hex(b))
    for op in ("sqr", "neg", "canon"):
        for a in F.row_values(op):
            r = F.row_expect(op, a)
            assert 0 <= r < R and r % P == F.row_residue(op, a)
    assert {0, P, 1, P - 1, 2 * P - R} <= set(F.row_values("is_zero"))
    assert {0, P - 1, P, P + 1, R - 1} <= set(F.row_values("canon"))
    assert {P, P + 1, R - 1, R - P} <= {a for a, _ in F.row_pairs("mul")}


def test_row_wave_cases_rotate_the_worst_pair_through_a_wave():
    for op in ("mul", "add", "sub", "canon"):
        cases, worst = F.row_wave_cases(op), F.row_worst(op)
        assert len(cases) == 16 and sum(F.row_passes(op, *worst)) >= 8
        for wave in range(4):
            rows = cases[4 * wave: 4 * wave + 4]
            assert rows[wave] == worst and sorted(map(str, rows)) == sorted(map(str, cases[:4]))
        assert F.row_pairs(op)[:16] == cases if op != "canon" else F.row_values(op)[:16] == tuple(a for a, _ in cases)


# ------------------------------------------------------------------ wnaf5
def test_wnaf_scalars():
    s = F.wnaf_scalars()
    assert set((0, 1, 15, 16, 17, 31, 2**255, N - 1, N, R - 1)) <= set(s) and len(s) == 10 + 5 + 64
    for k in s:
        d = F.EC.naf5(k)
        assert len(d) == F.EC.NAF_LEN and sum(v << i for i, v in enumerate(d)) == k


# ------------------------------------------------------------------ through the Shamir kernels
def test_combine_cases():
    lams = F.combine_lambda_cases()
    r2 = R * R % N
    in_win = [(name, T, lam) for name, T, lam in lams if F.in_window(T, N)]
    assert len(in_win) == 19 and any(T >= R for _, T, _ in lams)
    second_window = second_high = 0
    for name, T, lam in lams:
        assert 0 < lam < N and F.mul_T(lam, r2, N) == T
        lm = lam * R % N
        for yname, T2, y in F.combine_share_cases(lam):
            assert 0 < y < N and F.mul_T(lm, y, N) == T2, (name, yname)
            second_window += F.in_window(T2, N)
            second_high += T2 >= R
            # a lambda whose own T is in the window leaves lm < 2^256 - n: no second T >= 2^256
            assert not (F.in_window(T, N) and T2 >= R)
    assert second_window >= 100 and second_high >= 6
    both = sum(1 for name, T, lam in in_win for _, T2, _ in F.combine_share_cases(lam) if F.in_window(T2, N))
    assert both >= 50                                   # both products of one lane decided by the borrow


def test_deal_cases():
    assert F.DEAL_XS == (1, 2, 2**32 - 1) and F.DEAL_UNREACHABLE_XS == (1,)
    # x = 1: sc_mul(c1, R mod n) has T = c1 < n whatever c1 is
    assert F.deal_cases(1) == ()
    assert all(F.mul_T(c1, R % N, N) == c1 for c1, _ in F.random_pairs(N)[:200])
    for x in (2, 2**32 - 1):
        cases = F.deal_cases(x)
        assert sum(1 for _, T, _ in cases if F.in_window(T, N)) >= 8
        for name, T, c1 in cases:
            assert 0 < c1 < N and F.mul_T(c1, x * R % N, N) == T, (x, name)
    assert [name for name, _, _ in F.deal_cases(2**32 - 1)][:5] == ["n+1", "n+2^32", "2^256-1", "2^256", "2^256+1"]
