"""Exact integer models of the 256-bit field layers (flamingo_amd/csrc/flm_fe256.h, flm_fe_row.h) and
the operands that steer single field operations into the branches no ladder or Horner loop reaches.
No test functions: the premises are checked without a GPU by tests/test_fe_cases_cpu.py, the device
code against the lists by tests/test_fe_ops_gpu.py, through the test-only harness
tests/fieldtest/flm_fieldtest.hip (one operation per kernel) and, where an entry point gives control
of the operands, through flm_shamir_combine and flm_shamir_deal.  Every expected value is a Python
integer expression (a b R^-1 mod m and so on); the models only say which branch an operand takes.

Models, written from the headers, limb for limb:

* mul_columns(a, b): fe_mul's product scanning: per column K = 0..14 a 64-bit accumulator and the
  count of its carry-outs.  A column of n products (each at most 2^64 - 2^33 + 1) with a carry-in
  below (n + 1) 2^32 stays below n 2^64 for n >= 2, so the count is at most n - 1; column 0 has no
  carry-in and column 14 is bounded by a b < 2^512, so both count 0.  MUL_MAX_COUNT states that.
* sqr_columns(a): sqr_cols: the doubled cross sum with its three events per column: "shift" (the top
  bit of the 64-bit cross sum moved into the carry word by the doubling), "addc" (x + c overflows 64
  bits: `xh += (n < x)`) and "diag" (adding the diagonal product a_(K/2)^2 carries).
* mont_reduce_T(t): mont_reduce's signed column pass: (T, carry) with T the 256-bit value handed to
  mod_reduce_once and carry its ninth word, T + carry 2^256 = (t + M p) / 2^256.
* sc_mul_T(a, b): sc_mul's CIOS: (t, t8) before mod_reduce_once.
* the row layer is tools/ec_row_model.py (row_mul, row_add, row_sub, row_canon, row_is_zero).

The reduction window.  mod_reduce_once takes t - m when `t8 || !borrow`.  T = (a b + M m) / 2^256
lies in [m, 2^256), where the borrow alone decides, for about one product in 2^32; solve_window(T, b,
m) finds a < m with exactly that T: M = T 2^256 m^-1 (mod b) taken in (T 2^256 / m - b, 2^256), then
a = (T 2^256 - M m) / b.  window_targets(m) are m + 1, m + 2^32, 2^256 - 1, 2^256, 2^256 + 1 and 16
seeded values inside [m + 1, 2^256): 21 per modulus, 19 of them in the window.
  - fe_mul, sc_mul (mul_window_cases): b seeded random (the first that solves); all 21 are solved.
  - to_mont mod p and the scalar-field entry sc_mul(a, R^2 mod n) of the Shamir kernels
    (to_mont_window_cases): b is fixed; to_mont_unsolved(m) names the targets with no solution:
    2^256 - 1, 2^256 and one seeded value mod p (R^2 mod p is about 2^226.3, and a target p + d needs
    d below about b), 2^256 mod n.  The other 18 and 20 are solved.
  - from_mont: b = 1, T = (a + M p) / 2^256 < p + 1 and T = p only for a = 0 (where M = 0 and T = 0): no
    target is reachable, and FROM_MONT_REACHABLE is empty.  The list holds the solved to_mont
    results and the structured values instead, and the CPU test asserts the window is not reached.
  - fe_sqr: a^2 = r 2^256 (mod p) for small r gives T = r or p + r; sqr_window_cases() keeps the
    first 24 roots with T = p + r, and tries the five fixed targets: sqr_unsolved() names the one
    that is not a square, 2^256 - 1; p + 1, p + 2^32, 2^256 and 2^256 + 1 are solved.
  - T = m exactly needs a b = 0 (mod m): unreachable below m with non-zero operands.  sc_mul reaches it
    with the unreduced a = n (T = n, result 0), which the kernels may pass (sc_mul(lambda, R^2) takes
    lambda as loaded); a = 2^256 - 1 rides along, T < 2n still holding.

fe_sqr events: sqr_event_cases() holds for each column one witness per reachable event and one input
with none; SQR_UNREACHABLE gives the reason for the rest:
  - column 0: no cross products and no carry-in, and a_0^2 < 2^64: none of the three;
  - odd columns: no diagonal product, so no "diag";
  - column 14: no cross products (x = 0, so neither "shift" nor "addc"), and a^2 < 2^512 bounds
    c + a_7^2 below 2^64, so no "diag".

Row layer: ROW_MAX_PASSES records the largest counts of carry passes a structured search of the model
reaches (see tools/ec_row_model.py's docstring); row_pass_witnesses() has one operand pair per count.
In the harness element i sits in row i % 4 of wave i / 4, so row_wave_cases() puts the witness with
the most passes beside a one-pass operand, zero and p in each of the four rows of a wave.
"""
from __future__ import annotations

import functools
import os
import random
import sys

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _d in ("oracle", "tools", "tests"):
    if os.path.join(_ROOT, _d) not in sys.path:
        sys.path.insert(0, os.path.join(_ROOT, _d))

import ec_cases as EC  # noqa: E402
import ec_row_model as RM  # noqa: E402

P, N = EC.P, EC.N
R = 2**256
M32, M64 = (1 << 32) - 1, (1 << 64) - 1
N0 = 0xEE00BC4F                      # kN0 = -n^-1 mod 2^32
assert (N * N0 + 1) % 2**32 == 0 and (P + 1) % 2**32 == 0


def limbs(x: int, n: int = 8) -> list:
    return [(x >> (32 * i)) & M32 for i in range(n)]


def val(w) -> int:
    return sum(int(v) << (32 * i) for i, v in enumerate(w))


def mod_name(m: int) -> str:
    return {P: "p", N: "n"}[m]


# ------------------------------------------------------------------ fe_mul, fe_sqr, mont_reduce
def _col_range(K: int):
    return (0 if K < 8 else K - 7), (K if K < 8 else 7)


MUL_MAX_COUNT = [0 if K in (0, 14) else _col_range(K)[1] - _col_range(K)[0] for K in range(15)]   # n - 1


def mul_columns(a: int, b: int):
    """mul_cols: (t[16], the carry count of every column 0..14)"""
    la, lb = limbs(a), limbs(b)
    acc, t, counts = 0, [], []
    for K in range(15):
        lo, top = _col_range(K)
        hi = 0
        for i in range(lo, top + 1):
            acc += la[i] * lb[K - i]
            hi += acc >> 64
            acc &= M64
        t.append(acc & M32)
        counts.append(hi)
        acc = (acc >> 32) | (hi << 32)
    assert acc <= M32
    t.append(acc)
    return t, counts


def sqr_columns(a: int):
    """sqr_cols: (t[16], the set of events of every column 0..14)"""
    la = limbs(a)
    c, t, events = 0, [], []
    for K in range(15):
        lo, top = (0 if K < 8 else K - 7), (K - 1) // 2 if K >= 1 else -1
        x, xh, ev = 0, 0, set()
        for i in range(lo, top + 1):
            x += la[i] * la[K - i]
            xh += x >> 64
            x &= M64
        if x >> 63:
            ev.add("shift")
        xh = ((xh << 1) | (x >> 63)) & M32
        x = (x << 1) & M64
        n = (x + c) & M64
        if n < x:
            ev.add("addc")
            xh += 1
        x = n
        if K % 2 == 0:
            x += la[K // 2] ** 2
            if x >> 64:
                ev.add("diag")
                xh += 1
            x &= M64
        assert xh <= M32
        t.append(x & M32)
        c = (x >> 32) | (xh << 32)
        events.append(frozenset(ev))
    assert c <= M32
    t.append(c)
    return t, events


def mont_reduce_T(t):
    """mont_reduce's column pass on the 16 limbs t: (T, carry), the arguments of mod_reduce_once"""
    m, out, carry = [0] * 8, [0] * 8, 0
    for i in range(16):
        s = t[i] + carry
        if 3 <= i < 11:
            s += m[i - 3]
        if 6 <= i < 14:
            s += m[i - 6]
        if 7 <= i < 15:
            s -= m[i - 7]
        if i >= 8:
            s += m[i - 8]
        if i < 8:
            m[i] = s & M32
        else:
            out[i - 8] = s & M32
        carry = s >> 32                     # arithmetic, as the kernel's int64
    assert (val(out) + carry * R) * R == val(t) + val(m) * P
    return val(out), carry


def reduce_once(T: int, t8: int, m: int) -> int:
    """mod_reduce_once: t - m when t8 is set or the subtraction does not borrow"""
    return (T - m) % R if (t8 or T >= m) else T


def fe_mul_T(a: int, b: int) -> int:
    """T + carry 2^256 of fe_mul(a, b), by the column models"""
    t, _ = mul_columns(a, b)
    assert val(t) == a * b
    T, c = mont_reduce_T(t)
    return T + c * R


def fe_sqr_T(a: int) -> int:
    t, _ = sqr_columns(a)
    assert val(t) == a * a
    T, c = mont_reduce_T(t)
    return T + c * R


def fe_mul_model(a: int, b: int) -> int:
    T = fe_mul_T(a, b)
    return reduce_once(T % R, T >> 256, P)


def fe_sqr_model(a: int) -> int:
    T = fe_sqr_T(a)
    return reduce_once(T % R, T >> 256, P)


# ------------------------------------------------------------------ sc_mul
def sc_mul_T(a: int, b: int):
    """sc_mul's CIOS: (t, t8) before mod_reduce_once"""
    la, lb, ln = limbs(a), limbs(b), limbs(N)
    t, t8 = [0] * 8, 0
    for i in range(8):
        c = 0
        for j in range(8):
            c = la[j] * lb[i] + t[j] + (c >> 32)
            assert c <= M64
            t[j] = c & M32
        s = t8 + (c >> 32)
        hi0, hi1 = s & M32, s >> 32
        m = (t[0] * N0) & M32
        c = m * ln[0] + t[0]
        for j in range(1, 8):
            c = m * ln[j] + t[j] + (c >> 32)
            assert c <= M64
            t[j - 1] = c & M32
        s = hi0 + (c >> 32)
        t[7] = s & M32
        t8 = hi1 + (s >> 32)
    return val(t), t8


def sc_mul_model(a: int, b: int) -> int:
    T, t8 = sc_mul_T(a, b)
    return reduce_once(T, t8, N)


def mul_T(a: int, b: int, m: int) -> int:
    """T (with its ninth word) of the Montgomery product mod m by the layer's own model"""
    if m == P:
        return fe_mul_T(a, b)
    T, t8 = sc_mul_T(a, b)
    return T + t8 * R


def in_window(T: int, m: int) -> bool:
    return m <= T < R


# ------------------------------------------------------------------ structured values and pairs
@functools.lru_cache(maxsize=None)
def structured_values(m: int) -> tuple:
    """about 40 values below m with edge limbs"""
    v = [0, 1, 2, m - 1, m - 2, (m - 1) // 2, (m + 1) // 2]
    v += [2**(32 * k) for k in range(1, 8)] + [2**(32 * k) - 1 for k in range(1, 8)]
    v += [M32 << (32 * k) for k in range(8)]
    v += [R - 2**224 - 1, R % m, R * R % m, m - R % m]
    out = []
    for x in v:
        assert 0 <= x < m, hex(x)
        if x not in out:
            out.append(x)
    return tuple(out)


N_RANDOM = 2000


@functools.lru_cache(maxsize=None)
def random_pairs(m: int) -> tuple:
    rng = random.Random(256000 + (m == N))
    return tuple((rng.randrange(m), rng.randrange(m)) for _ in range(N_RANDOM))


@functools.lru_cache(maxsize=None)
def structured_pairs(m: int) -> tuple:
    """all pairs of structured_values(m), then the 2,000 seeded random pairs"""
    s = structured_values(m)
    return tuple((a, b) for a in s for b in s) + random_pairs(m)


@functools.lru_cache(maxsize=None)
def unary_values(m: int) -> tuple:
    """structured values and the first operands of the random pairs (all below m)"""
    return structured_values(m) + tuple(a for a, _ in random_pairs(m))


@functools.lru_cache(maxsize=None)
def range_values(m: int) -> tuple:
    """inputs of the comparisons with m (fe_lt_p, sc_lt_n, sc_below_n): anything below 2^256"""
    rng = random.Random(256010 + (m == N))
    edge = (m, m + 1, m + 2, R - 1, R - 2, m + 2**32, m - 2**32, m + 2**224 - 2**193, 2**255, m ^ (1 << 255))
    # one limb of m lowered or raised by one, the others kept: the borrow chain decides at every position
    per_limb = tuple(x for k in range(8) for x in (m - (1 << (32 * k)), m + (1 << (32 * k))) if 0 <= x < R)
    return structured_values(m) + edge + per_limb + tuple(rng.getrandbits(256) for _ in range(500))


# ------------------------------------------------------------------ fe_mul's carry counts
@functools.lru_cache(maxsize=None)
def mul_count_cases() -> tuple:
    """(K, kind, a, b, count): for every column one pair with the largest carry count (all-ones limbs
    in the column's products, the top limb 0xfffffffe to stay below p) and one with count 0 everywhere
    (16-bit limbs)."""
    rng = random.Random(256020)
    out = []
    for K in range(15):
        lo, top = _col_range(K)
        la, lb = [0] * 8, [0] * 8
        for i in range(lo, top + 1):
            la[i] = lb[K - i] = M32
        if la[7]:
            la[7] -= 1
        if lb[7]:
            lb[7] -= 1
        a, b = val(la), val(lb)
        out.append((K, "max", a, b, mul_columns(a, b)[1][K]))
        a, b = (val([rng.randrange(1, 1 << 16) for _ in range(8)]) for _ in range(2))
        out.append((K, "zero", a, b, mul_columns(a, b)[1][K]))
    return tuple(out)


# ------------------------------------------------------------------ the reduction window
def window_targets(m: int) -> tuple:
    rng = random.Random(256030 + (m == N))
    return (m + 1, m + 2**32, R - 1, R, R + 1) + tuple(rng.randrange(m + 1, R) for _ in range(16))


def target_name(T: int, m: int) -> str:
    s = mod_name(m)
    return {m + 1: f"{s}+1", m + 2**32: f"{s}+2^32", R - 1: "2^256-1", R: "2^256", R + 1: "2^256+1"}.get(
        T, f"{s}+0x{T - m:x}")


def solve_window(T: int, b: int, m: int):
    """a < m with (a b + M m) / 2^256 == T, or None: M = T 2^256 m^-1 (mod b), the largest such
    value below 2^256 and not above T 2^256 / m, which must stay above T 2^256 / m - b"""
    if b <= 0:
        return None
    top = min(R - 1, T * R // m)
    r = T * R * pow(m, -1, b) % b if b > 1 else 0
    M = top - (top - r) % b
    if M < 0:
        return None
    num = T * R - M * m
    if num < 0 or num % b:
        return None
    a = num // b
    return a if 0 <= a < m else None


@functools.lru_cache(maxsize=None)
def mul_window_cases(m: int) -> tuple:
    """(target name, T, a, b) for every window target, b the first seeded random value that solves it"""
    rng = random.Random(256040 + (m == N))
    out = []
    for T in window_targets(m):
        for _ in range(64):
            b = rng.randrange(1, m)
            a = solve_window(T, b, m)
            if a is not None:
                break
        assert a is not None, target_name(T, m)
        out.append((target_name(T, m), T, a, b))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def fixed_b_window_cases(b: int, m: int) -> tuple:
    """(target name, T, a or None) for every window target with the second operand fixed"""
    return tuple((target_name(T, m), T, solve_window(T, b, m)) for T in window_targets(m))


def to_mont_window_cases(m: int) -> tuple:
    """the entry into Montgomery form: to_mont (m = p) and sc_mul(a, R^2 mod n)"""
    return fixed_b_window_cases(R * R % m, m)


def to_mont_unsolved(m: int) -> tuple:
    return tuple(name for name, _, a in to_mont_window_cases(m) if a is None)


FROM_MONT_REACHABLE = ()         # b = 1: T <= p, and T = p only for a = 0 where T = 0


@functools.lru_cache(maxsize=None)
def from_mont_values() -> tuple:
    """from_mont's inputs: the structured and random values and every solved to_mont result"""
    solved = tuple(a * R % P for _, _, a in to_mont_window_cases(P) if a is not None)
    return unary_values(P) + solved


def sqrt_p(x: int):
    r = pow(x, (P + 1) // 4, P)
    return r if r * r % P == x % P else None


SQR_WINDOW_SMALL = 24


@functools.lru_cache(maxsize=None)
def sqr_window_cases() -> tuple:
    """(name, T, a): squares whose T lies in the window: the first SQR_WINDOW_SMALL roots of r 2^256
    for small r, and the fixed targets T = p + r that are squares (None otherwise)"""
    out, r = [], 0
    while len(out) < SQR_WINDOW_SMALL:
        r += 1
        s = sqrt_p(r * R % P)
        for a in ((s, P - s) if s is not None else ()):
            if fe_sqr_T(a) == P + r:
                out.append((f"p+{r}", P + r, a))
    del out[SQR_WINDOW_SMALL:]
    for T in window_targets(P)[:5]:
        s, hit = sqrt_p((T - P) * R % P), None
        for a in ((s, P - s) if s is not None else ()):
            if fe_sqr_T(a) == T:
                hit = a
        out.append((target_name(T, P), T, hit))
    return tuple(out)


def sqr_unsolved() -> tuple:
    return tuple(name for name, _, a in sqr_window_cases() if a is None)


@functools.lru_cache(maxsize=None)
def sc_mul_unreduced_cases() -> tuple:
    """(a, b) with the first operand not below n: a = n (T = n exactly, result 0) and a = 2^256 - 1"""
    rng = random.Random(256050)
    bs = (1, 2, N - 1, R * R % N, R % N) + tuple(rng.randrange(1, N) for _ in range(8))
    return tuple((a, b) for a in (N, R - 1, N + 1) for b in bs)


# ------------------------------------------------------------------ fe_sqr's events
SQR_EVENTS = ("shift", "addc", "diag")
SQR_UNREACHABLE = {}
for _K in range(15):
    for _e in SQR_EVENTS:
        if _K == 0:
            SQR_UNREACHABLE[(_K, _e)] = "column 0 has no cross products and no carry-in, and a_0^2 < 2^64"
        elif _K == 14:
            SQR_UNREACHABLE[(_K, _e)] = ("column 14 has no cross products, so x = 0" if _e != "diag"
                                         else "a^2 < 2^512 bounds c + a_7^2 below 2^64")
        elif _e == "diag" and _K % 2:
            SQR_UNREACHABLE[(_K, _e)] = "an odd column has no diagonal product"

_SQR_SPECIAL = (0x80000001, 0xFFFFFFFE, 0xFFFFFFFF, 0x80000000, 0xB504F334, 0xB504F333, 0x7FFFFFFF, 0xC0000000,
                0xAAAAAAAB, 1, 2, 3)


def _sqr_candidates(K: int, rng):
    """Directed candidates for column K: the limbs of its cross products and of column K - 1 (whose
    sum is the carry-in c) from special values, the rest zero; a pair a_i a_j just below 2^63, so that
    its double is just below 2^64 and any carry-in overflows it (the issue's a_0 a_1 witness moved up
    the columns)."""
    lo, top = (0 if K < 8 else K - 7), (K - 1) // 2
    used = sorted({i for i in range(lo, top + 1)} | {K - i for i in range(lo, top + 1)} |
                  {i for i in range(8) if 0 <= K - 1 - i < 8})
    while True:
        la = [0] * 8
        mode = rng.randrange(3)
        for i in used:
            la[i] = rng.choice(_SQR_SPECIAL) if mode < 2 else rng.getrandbits(32)
        if mode == 1 and top >= lo:
            i = rng.randrange(lo, top + 1)
            la[i] = rng.randrange(1 << 31, 1 << 32)
            la[K - i] = ((1 << 63) - 1) // la[i]
            for j in range(lo, top + 1):
                if j != i and rng.randrange(2):
                    la[j] = 0
        a = val(la)
        if 0 < a < P:
            yield a


@functools.lru_cache(maxsize=None)
def sqr_event_cases() -> tuple:
    """(K, event or "none", a): for every column one witness per reachable event, and one input
    whose column K has none; found by a seeded directed search of the model (bounded tries)."""
    out = []
    for K in range(15):
        rng = random.Random(256100 + K)
        want = {e for e in SQR_EVENTS if (K, e) not in SQR_UNREACHABLE} | {"none"}
        gen = _sqr_candidates(K, rng) if K >= 1 else iter([1, M32, 0x12345678])
        for _, a in zip(range(20000), gen):
            if not want:
                break
            ev = sqr_columns(a)[1][K]
            for e in sorted(want):
                if (e == "none" and not ev) or e in ev:
                    out.append((K, e, a))
                    want.discard(e)
        assert not want, (K, want)
    return tuple(out)


# ------------------------------------------------------------------ add, subtract, negate
@functools.lru_cache(maxsize=None)
def add_edge_cases(m: int) -> tuple:
    """(a, b) below m with a + b in m - 1, m, m + 1, 2^256 - 1, 2^256, 2^256 + 1, several splits of each"""
    rng = random.Random(256200 + (m == N))
    out = []
    for s in (m - 1, m, m + 1, R - 1, R, R + 1):
        lo, hi = max(0, s - (m - 1)), min(m - 1, s)
        for a in (lo, hi, s // 2, s - s // 2, lo + 1, rng.randrange(lo, hi + 1), rng.randrange(lo, hi + 1)):
            assert 0 <= a < m and 0 <= s - a < m
            out.append((a, s - a))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def sub_edge_cases(m: int) -> tuple:
    """a = b, a = b - 1, a = 0, b = 0 over the structured values"""
    out = []
    for v in structured_values(m):
        out += [(v, v), (0, v), (v, 0)]
        if v:
            out.append((v - 1, v))
    return tuple(out)


# ------------------------------------------------------------------ the row layer
ROW_EDGE = (0, 1, 2, P - 1, P, P + 1, R - 1, R - P, 2 * P - R, R - 2, 2**255, 2**224, 2**96 - 1, 2**192, 2**128 + 1)


@functools.lru_cache(maxsize=None)
def row_search_values() -> tuple:
    """The structured search's operands: the edge values and limb patterns whose products, sums and
    differences carry along the row (runs of all-ones limbs under a low carry, a single bit per limb,
    p's own limbs shifted)."""
    v = list(ROW_EDGE)
    for k in range(8):
        v += [M32 << (32 * k), 1 << (32 * k), (1 << (32 * k)) - 1 if k else 3, R - (1 << (32 * k)),
              (R - 1) ^ (M32 << (32 * k)), 0x80000000 << (32 * k), R - 1 - (1 << (32 * k))]
    v += [P - 2**32, P + 2**32, P - 2**96, P + 2**96 - 1, R - 2**224, R - 2**224 - 1, R - 2**192, 2**224 - 2**192,
          2**224 - 2**192 - 2**96 + 1, R - (2**224 - 2**192 - 2**96 + 1), (R - 1) // 3, (R - 1) // 5, (R - 1) // 0xFFFF,
          2**128 - 1, 2**128, 2**160 - 1, R - 2**128, R - 2**96, R - 2**32 - 1, 0xFFFFFFFE00000001, 0xFFFFFFFF00000001]
    out = []
    for x in v:
        assert 0 <= x < R
        if x not in out:
            out.append(x)
    return tuple(out)


def row_passes(op: str, a: int, b: int = 0) -> tuple:
    """the model's pass counts of one row operation: (column passes, fold passes) for mul and sqr,
    (fold passes,) for add, sub and neg, (borrow passes,) for canon"""
    if op == "mul":
        return RM.row_mul(a, b)[1:]
    if op == "sqr":
        return RM.row_mul(a, a)[1:]
    if op == "add":
        return RM.row_add(a, b)[1:]
    if op == "sub":
        return RM.row_sub(a, b)[1:]
    if op == "neg":
        return RM.row_sub(0, a)[1:]
    assert op == "canon"
    return RM.row_canon(a)[1:]


def row_expect(op: str, a: int, b: int = 0) -> int:
    """the model's lazy result (bit for bit what the kernel must return); checked mod p by the CPU test"""
    if op == "is_zero":
        return int(RM.row_is_zero(a))
    return {"mul": lambda: RM.row_mul(a, b), "sqr": lambda: RM.row_mul(a, a), "add": lambda: RM.row_add(a, b),
            "sub": lambda: RM.row_sub(a, b), "neg": lambda: RM.row_sub(0, a), "canon": lambda: RM.row_canon(a)}[op]()[0]


def row_residue(op: str, a: int, b: int = 0) -> int:
    return {"mul": a * b, "sqr": a * a, "add": a + b, "sub": a - b, "neg": -a, "canon": a}[op] % P


@functools.lru_cache(maxsize=None)
def row_pass_search() -> dict:
    """{(op, which, count): (a, b)}: the first operand pair of the structured search (all pairs of
    row_search_values) for every count of passes; which is "columns" or "fold" ("borrow" for canon)."""
    vals, found = row_search_values(), {}
    for a in vals:
        for b in vals:
            p1, p2 = RM.row_mul(a, b)[1:]
            found.setdefault(("mul", "columns", p1), (a, b))
            found.setdefault(("mul", "fold", p2), (a, b))
            found.setdefault(("add", "fold", RM.row_add(a, b)[1]), (a, b))
            found.setdefault(("sub", "fold", RM.row_sub(a, b)[1]), (a, b))
        found.setdefault(("canon", "borrow", RM.row_canon(a)[1]), (a, 0))
    return found


def row_max_passes() -> dict:
    out = {}
    for (op, which, n) in row_pass_search():
        out[(op, which)] = max(out.get((op, which), 0), n)
    return out


# what the search reaches; tools/ec_row_model.py's docstring quotes these, test_fe_cases_cpu.py asserts them
ROW_MAX_PASSES = {("mul", "columns"): 7, ("mul", "fold"): 11, ("add", "fold"): 11, ("sub", "fold"): 11,
                  ("canon", "borrow"): 8}


def row_pass_witnesses(op: str) -> tuple:
    """(a, b) for every pass count the search reaches in `op` (either loop)"""
    return tuple(dict.fromkeys(ab for (o, _, _), ab in sorted(row_pass_search().items()) if o == op))


def row_worst(op: str) -> tuple:
    """the pair with the most passes in total"""
    return max(row_pass_witnesses(op), key=lambda ab: sum(row_passes(op, *ab)))


def row_wave_cases(op: str) -> tuple:
    """16 elements, four waves: the worst pair with a one-pass pair, zero and p as its wave's other
    rows, rotated through the four row positions"""
    quiet = {"mul": (3, 5), "add": (1, 2), "sub": (5, 3), "canon": (R - 1, 0)}[op]
    assert max(row_passes(op, *quiet)) <= 1
    base = [row_worst(op), quiet, (0, 0), (P, P if op != "canon" else 0)]
    return tuple(base[(i - rot) % 4] for rot in range(4) for i in range(4))


@functools.lru_cache(maxsize=None)
def row_pairs(op: str) -> tuple:
    """the two-operand row list (mul, add, sub): the wave rotations first (they rely on element i
    being row i % 4 of wave i / 4), the pass witnesses, all pairs of the edge values, random pairs
    anywhere in [0, 2^256)"""
    rng = random.Random(256300)
    rand = tuple((rng.getrandbits(256), rng.getrandbits(256)) for _ in range(600))
    return row_wave_cases(op) + row_pass_witnesses(op) + tuple((a, b) for a in ROW_EDGE for b in ROW_EDGE) + rand


@functools.lru_cache(maxsize=None)
def row_values(op: str) -> tuple:
    """the one-operand row list (sqr, neg, canon, is_zero)"""
    rng = random.Random(256310)
    head = tuple(a for a, _ in row_wave_cases("canon")) if op == "canon" else ()
    wit = {"sqr": "mul", "neg": "sub", "canon": "canon", "is_zero": "canon"}[op]
    mid = tuple(x for ab in row_pass_witnesses(wit) for x in ab)
    return head + mid + row_search_values() + tuple(rng.getrandbits(256) for _ in range(400))


# ------------------------------------------------------------------ wnaf5
@functools.lru_cache(maxsize=None)
def wnaf_scalars() -> tuple:
    rng = random.Random(256400)
    alt = (int("55" * 32, 16), int("aa" * 32, 16), int("0f" * 32, 16), int("f0" * 32, 16), int("3c" * 32, 16))
    return (0, 1, 15, 16, 17, 31, 2**255, N - 1, N, R - 1) + alt + tuple(rng.getrandbits(256) for _ in range(64))


# ------------------------------------------------------------------ through the Shamir kernels
# shamir_combine_kernel, T = 1: lm = sc_mul(lambda, R^2 mod n), then sc_mul(lm, y).  A lambda whose
# entry product has T = n + d in the window leaves lm = d < 2^256 - n, and the second product's T can
# then reach n + d2 only for d2 below about lm: its window, never T >= 2^256.  So the y with T >= 2^256
# ride on other lambdas: the one solved for the entry target 2^256 + 1 (its own T has the ninth word
# set) and seeded random ones.
# shamir_deal_kernel, T = 2: acc = sc_mul(c1, x R mod n) + c0.  For x = 1 the second operand is R mod n
# = 2^256 - n and T 2^256 = c1 (2^256 - n) + M n has the one solution M = c1, T = c1 < n: no window
# target is reachable (DEAL_UNREACHABLE_XS); x = 2 and x = 2^32 - 1 reach it.
DEAL_XS = (1, 2, 2**32 - 1)
DEAL_UNREACHABLE_XS = (1,)
COMBINE_RANDOM_LAMBDAS = 3


@functools.lru_cache(maxsize=None)
def combine_lambda_cases() -> tuple:
    """(name, T, lambda): lambda < n whose entry product sc_mul(lambda, R^2 mod n) has T on every
    window target that has a solution, then COMBINE_RANDOM_LAMBDAS seeded random ones (T as it falls)"""
    rng = random.Random(256500)
    out = [(name, T, a) for name, T, a in to_mont_window_cases(N) if a is not None]
    for i in range(COMBINE_RANDOM_LAMBDAS):
        lam = rng.randrange(N >> 1, N)
        out.append((f"random {i}", mul_T(lam, R * R % N, N), lam))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def combine_share_cases(lam: int) -> tuple:
    """(target name, T, y): y < n whose product sc_mul(lambda R mod n, y) has T on target, for every
    target that has a solution with this lambda"""
    return tuple((name, T, y) for name, T, y in fixed_b_window_cases(lam * R % N, N) if y is not None)


@functools.lru_cache(maxsize=None)
def deal_cases(x: int) -> tuple:
    """(target name, T, c1): top coefficients c1 < n whose Horner product sc_mul(c1, x R mod n) has T on target"""
    return tuple((name, T, a) for name, T, a in fixed_b_window_cases(x * R % N, N) if a is not None)
