"""Deterministic edge inputs for the P-256 kernels (flamingo_amd/csrc/flm_p256.hip over flm_fe256.h, flm_jac256.h and flm_fe_row.h) and
their expected results from the big-int oracle (oracle/ec_oracle.py).  No test functions: the
premises are checked without a GPU by tests/test_ec_cases_cpu.py, the kernels against them by
tests/test_ec_edges_gpu.py.

* naf5 / chain_events restate the kernels' width-5 NAF recoding (wnaf5) and their most-significant-
  first accumulate loop, and say at which step an addition meets acc == Q (the "double" branch of
  jac_add, coop_add_w level 6 and RowField::dbl) or acc == -Q (the result is infinity).
* structured_points: affine points whose abscissa has limbs of all zeros / all ones / a single bit,
  in normal form (what the row kernel multiplies) and in Montgomery form (what every other kernel
  multiplies, x R mod p with R = 2^256).
* pool: 257 random points with random 256-bit scalars and their products, for the batch-shape tests.
* the case lists of the GPU tests.  Every expected value is computed once per process: products go
  through one memo (mulc), so a point and scalar shared by two lists cost one oracle multiplication.
"""
from __future__ import annotations

import functools
import hashlib
import os
import random
import sys
from collections import namedtuple

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if os.path.join(_ROOT, "oracle") not in sys.path:
    sys.path.insert(0, os.path.join(_ROOT, "oracle"))

import ec_oracle as E  # noqa: E402

P, N = E.P, E.N
R = 2**256
R_INV = pow(R, -1, P)
NAF_LEN = 258          # kNafLen
ZERO_SEED = hashlib.sha256(bytes(64)).digest()


# ------------------------------------------------------------------ the wNAF chain
def naf5(k: int) -> list:
    """wnaf5 of flm_jac256.h: NAF_LEN digits, least significant first, each 0 or odd in [-15, 15]."""
    assert 0 <= k < 2**256
    d = []
    for _ in range(NAF_LEN):
        v = 0
        if k & 1:
            v = k & 31
            if v >= 16:
                v -= 32
            k -= v
        d.append(v)
        k >>= 1
    assert k == 0
    return d


def chain_events(k: int) -> list:
    """The exceptional additions of the kernels' accumulate loop for scalar k and a point of order
    n: [(w, digit, kind)] for every digit position w (walked from NAF_LEN - 1 down) at which the
    accumulator m P meets the addend digit P with m == digit ("double") or m == -digit ("infinity")
    mod n.  The first non-zero digit only loads the accumulator."""
    d = naf5(k)
    m = None
    events = []
    for w in range(NAF_LEN - 1, -1, -1):
        if m is not None:
            m = 2 * m % N
        v = d[w]
        if not v:
            continue
        if m is None:
            m = v % N
            continue
        if m == v % N:
            events.append((w, v, "double"))
        elif m == -v % N:
            events.append((w, v, "infinity"))
        m = (m + v) % N
    return events


# ------------------------------------------------------------------ points
def lift_x(x: int):
    """(x mod p, y) with y = rhs^((p+1)/4) when rhs is a square, else None."""
    x %= P
    rhs = (x * x * x + E.A * x + E.B) % P
    y = pow(rhs, (P + 1) // 4, P)
    return (x, y) if y * y % P == rhs else None


def limb_candidates() -> list:
    """256-bit values with structured 32-bit limbs: small, just below p, 2^k, 2^k - 1, p - 2^k."""
    c = list(range(40)) + [P - 1 - i for i in range(40)]
    for k in range(0, 256, 32):
        c += [2**k, 2**k - 1, P - 2**k]
    seen, out = set(), []
    for v in c:
        if v not in seen:
            seen.add(v)
            out.append(v)
    return out


@functools.lru_cache(maxsize=None)
def structured_points() -> dict:
    """{"normal": [...], "mont": [...]}: the on-curve points of abscissa m (normal form: the limbs the
    row kernel sees) and m R^-1 mod p (the Montgomery limbs of the other kernels are then m), m over
    limb_candidates().  The first four of each family come with both signs of y."""
    out = {}
    for name, conv in (("normal", lambda m: m), ("mont", lambda m: m * R_INV % P)):
        pts = [pt for pt in (lift_x(conv(m)) for m in limb_candidates()) if pt is not None]
        out[name] = pts + [(x, P - y) for x, y in pts[:4]]
    return out


Pool = namedtuple("Pool", "points scalars products")


@functools.lru_cache(maxsize=None)
def _pool_all() -> Pool:
    rng = random.Random(20240607)
    pts, seen = [], set()
    while len(pts) < 257:
        pt = lift_x(rng.getrandbits(256))
        if pt is None or pt[0] in seen:
            continue
        seen.add(pt[0])
        pts.append(pt if rng.getrandbits(1) else (pt[0], P - pt[1]))
    ks = []
    while len(ks) < 257:
        k = rng.getrandbits(256)
        if k not in ks:
            ks.append(k)
    return Pool(pts, ks, [mulc(k, pt) for k, pt in zip(ks, pts)])


def pool(n: int = 257) -> Pool:
    """n distinct random points (a random abscissa lifted to the curve, random sign), n distinct random
    256-bit scalars (fixed seed) and the oracle's products; pool(n) is a prefix of pool(257)."""
    full = _pool_all()
    return Pool(full.points[:n], full.scalars[:n], full.products[:n])


# ------------------------------------------------------------------ expected values
@functools.lru_cache(maxsize=None)
def mulc(k: int, pt):
    """ec_oracle.mul, remembered."""
    return E.mul(k, pt)


def seed_of(pt) -> bytes:
    return hashlib.sha256(E.wire(pt)).digest()


def combine_expect(c1, shares_by_term, lambdas, negate=True):
    """ec_oracle.combine with its products taken from the memo (the same sum in the same order);
    tests/test_ec_cases_cpu.py checks it against ec_oracle.combine itself."""
    D = len(c1) if c1 is not None else len(shares_by_term[0])
    points = []
    for i in range(D):
        s = None
        for j, lam in enumerate(lambdas):
            s = E.add(s, mulc(lam, shares_by_term[j][i]))
        if negate:
            s = E.neg(s)
        points.append(E.add(c1[i], s) if c1 is not None else s)
    return points, [seed_of(pt) for pt in points]


# ------------------------------------------------------------------ 1. exceptional scalars
EXC_SCALARS = [N + 30, N, N + 1, N - 1, N + 15, N + 31, 15, 16, 30, 31, 32, 33, 2**255, 2**256 - 1]
# the only scalars of any list below whose chain meets an exceptional addition, and which one
EVENTS = {N + 30: "double", N: "infinity"}
RANDOM_SCALAR = 0x8F3A6C1E5D7B9204C6E8A0B2D4F61357_9BDF02468ACE13579BDF0246_8ACE1357


def exceptional_points() -> list:
    S = structured_points()
    return [E.G] + pool(3).points + [S["normal"][3], S["normal"][-1], S["mont"][7]]


@functools.lru_cache(maxsize=None)
def exceptional_cases():
    """(points, scalars, want): every exceptional_points() by every EXC_SCALARS."""
    pts, ks = [], []
    for pt in exceptional_points():
        for k in EXC_SCALARS:
            pts.append(pt)
            ks.append(k)
    return pts, ks, [mulc(k, pt) for k, pt in zip(ks, pts)]


# ------------------------------------------------------------------ 2. structured points
STRUCT_SCALARS = [1, 2, 3, 15, RANDOM_SCALAR, N - 1, 2**256 - 1]


@functools.lru_cache(maxsize=None)
def structured_cases(family: str):
    pts, ks = [], []
    for pt in structured_points()[family]:
        for k in STRUCT_SCALARS:
            pts.append(pt)
            ks.append(k)
    return pts, ks, [mulc(k, pt) for k, pt in zip(ks, pts)]


STRUCT_LAMBDAS = [RANDOM_SCALAR, N - 1, 3, 15]


@functools.lru_cache(maxsize=None)
def structured_combine(family: str):
    """(c1, shares, lambdas): a T = 4 combine (full Straus groups of 2 and 4) whose every share is a
    structured point; column i takes points i, i + 1, i + 2, i + 3 of the family and c1 the point
    i + 4, so the products are those of structured_cases."""
    S = structured_points()[family]
    D = len(S)
    shares = [[S[(i + j) % D] for i in range(D)] for j in range(4)]
    c1 = [S[(i + 4) % D] for i in range(D)]
    return c1, shares, list(STRUCT_LAMBDAS)


# ------------------------------------------------------------------ 4 / 5. combine shapes
COMBINE_SHAPES = [(1, 1), (2, 3), (3, 5), (5, 13), (7, 9), (8, 8), (9, 7), (16, 5), (17, 9)]
INSTANCE_SHAPE = (5, 70)


@functools.lru_cache(maxsize=None)
def combine_case(T: int, D: int):
    """(c1, shares, lambdas): random shares (pool points, distinct within a column) and random lambdas
    below n; the protocol's relation between them is not needed for a parity check."""
    rng = random.Random(1000 * T + D)
    pts = pool().points
    off = rng.randrange(257)
    shares = [[pts[(off + j * D + i) % 257] for i in range(D)] for j in range(T)]
    c1 = [pts[(off + 131 + 3 * i) % 257] for i in range(D)]
    return c1, shares, [rng.randrange(1, N) for _ in range(T)]


@functools.lru_cache(maxsize=None)
def combine_variants(T: int, D: int) -> dict:
    """{(with_c1, negate): (points, seeds)} of combine_case(T, D)."""
    c1, shares, lam = combine_case(T, D)
    return {(w, neg): combine_expect(c1 if w else None, shares, lam, neg) for w in (True, False) for neg in (True, False)}


# ------------------------------------------------------------------ 6. exceptional combines
ExcCombine = namedtuple("ExcCombine", "name c1 shares lambdas special want_points want_seeds")
EXC_D = 12
EXC_SPECIAL = (0, 5, 11)       # the exceptional columns; the other nine are ordinary
EXC_A = RANDOM_SCALAR >> 3     # below 2^253, so 2a is a scalar too


@functools.lru_cache(maxsize=None)
def exceptional_combines() -> list:
    """D = 12 batches in which columns EXC_SPECIAL meet an exceptional addition and the other columns
    are ordinary.  The lambdas are one per term, so each kind of case is its own batch."""
    pts = pool().points
    a = EXC_A
    b = pool().scalars[7] % N

    def base(T, off):
        return [[pts[(off + j * EXC_D + i) % 257] for i in range(EXC_D)] for j in range(T)]

    def c1_of(off):
        return [pts[(off + 200 + i) % 257] for i in range(EXC_D)]

    out = []

    def emit(name, c1, shares, lam):
        for tag, c in (("c1", c1), ("none", None)):
            if c is None and name.startswith("c1_"):
                continue
            want = combine_expect(c, shares, lam, True)
            out.append(ExcCombine(f"{name}-{tag}", c, shares, lam, EXC_SPECIAL, want[0], want[1]))

    # shares (P, P), lambdas (1, 1): P + P, a doubling in the Straus lane / in the finish tree
    sh = base(2, 0)
    for i in EXC_SPECIAL:
        sh[1][i] = sh[0][i]
    emit("equal_shares_unit", c1_of(0), sh, [1, 1])
    # shares (P, 2P), lambdas (2a, a): equal products under different Jacobian Z
    sh = base(2, 24)
    for i in EXC_SPECIAL:
        sh[1][i] = mulc(2, sh[0][i])
    emit("equal_products", c1_of(24), sh, [2 * a, a])
    # shares (P, P), lambdas (a, n - a): the sum is infinity
    sh = base(2, 48)
    for i in EXC_SPECIAL:
        sh[1][i] = sh[0][i]
    emit("opposite_products", c1_of(48), sh, [a, N - a])
    sh = base(2, 72)
    for i in EXC_SPECIAL:
        sh[1][i] = sh[0][i]
    emit("opposite_unit", c1_of(72), sh, [1, N - 1])
    # lambda 0 and lambda n (a valid 32-byte scalar congruent to 0): the term is infinity everywhere
    emit("lambda_zero", c1_of(96), base(2, 96), [0, b])
    emit("lambda_n", c1_of(120), base(2, 120), [N, b])
    # lambda n + 30: every column's first product ends on acc == Q inside the scalar multiplication (the
    # only way a combine reaches the doubling branch of coop_add_w: equal terms meet in the finish kernel)
    emit("lambda_n_plus_30", c1_of(120), base(2, 120), [N + 30, b])
    # T = 3 and c1 == sum (the result is infinity) / c1 == -sum (the result is 2 c1)
    lam3 = [pool().scalars[8] % N, pool().scalars[9] % N, pool().scalars[10] % N]
    sh = base(3, 144)
    s = combine_expect(None, sh, lam3, False)[0]
    c1 = c1_of(144)
    for i in EXC_SPECIAL:
        c1[i] = s[i]
    emit("c1_equals_sum", c1, sh, lam3)
    c1 = c1_of(144)
    for i in EXC_SPECIAL:
        c1[i] = E.neg(s[i])
    emit("c1_equals_minus_sum", c1, sh, lam3)
    # T = 1 and c1 == -lambda S: lane 0 of the finish kernel adds c1 (Z = 1) to an equal Jacobian point
    sh = base(1, 180)
    s = combine_expect(None, sh, [b], False)[0]
    c1 = c1_of(180)
    for i in EXC_SPECIAL:
        c1[i] = E.neg(s[i])
    emit("c1_doubles_in_finish", c1, sh, [b])
    return out


# ------------------------------------------------------------------ 7. bad inputs
def bad_wire_points() -> dict:
    """Wire encodings (64 bytes) that are not points of P-256, by name.  x_p and x_5_plus_p are
    congruent mod p to valid points (x = 0 and x = 5): only a range check rejects them."""
    def w(x, y):
        return x.to_bytes(32, "big") + y.to_bytes(32, "big")
    y0, y5 = lift_x(0)[1], lift_x(5)[1]
    top = 2**256 - 1
    lifted = lift_x(top)
    return {"y_plus_1": w(E.G[0], E.G[1] + 1),
            "x_p": w(P, y0),
            "x_all_ones": w(top, lifted[1] if lifted else E.G[1]),
            "x_5_plus_p": w(5 + P, y5),
            "zero_wire": bytes(64)}


FLAG_N = 9
MUL_BAD = {0: "y_plus_1", 3: "x_p", 4: "x_all_ones", 6: "zero_wire", 8: "x_5_plus_p"}
COMBINE_T = 3
C1_BAD = {0: "y_plus_1", 4: "x_5_plus_p", 6: "zero_wire"}
SHARE_BAD = {(0, 1): "y_plus_1", (1, 3): "x_p", (0, 4): "x_5_plus_p", (2, 8): "x_all_ones"}


@functools.lru_cache(maxsize=None)
def flag_mul_case():
    """(points wire (9 x 64 bytes), scalars, want): want[i] is None at the bad positions MUL_BAD."""
    p = pool(FLAG_N)
    bad = bad_wire_points()
    wires = [bad[MUL_BAD[i]] if i in MUL_BAD else E.wire(p.points[i]) for i in range(FLAG_N)]
    want = [None if i in MUL_BAD else p.products[i] for i in range(FLAG_N)]
    return wires, list(p.scalars), want


@functools.lru_cache(maxsize=None)
def flag_combine_case():
    """(c1 wires, share wires [T][D], lambdas, good columns, want points, want seeds): a T = 3, D = 9
    combine with c1 bad at C1_BAD and shares bad at SHARE_BAD; the expected values are those of the
    clean batch and hold at the columns without a bad input."""
    c1, shares, lam = combine_case(COMBINE_T, FLAG_N)
    want = combine_expect(c1, shares, lam, True)
    bad = bad_wire_points()
    c1_w = [bad[C1_BAD[i]] if i in C1_BAD else E.wire(c1[i]) for i in range(FLAG_N)]
    sh_w = [[bad[SHARE_BAD[(j, i)]] if (j, i) in SHARE_BAD else E.wire(shares[j][i]) for i in range(FLAG_N)]
            for j in range(COMBINE_T)]
    good = [i for i in range(FLAG_N) if i not in C1_BAD and i not in {c for _, c in SHARE_BAD}]
    return c1_w, sh_w, lam, good, want[0], want[1]


# ------------------------------------------------------------------ every scalar the GPU tests use
def gpu_scalars() -> list:
    ks = list(EXC_SCALARS) + list(STRUCT_SCALARS) + list(STRUCT_LAMBDAS) + list(pool().scalars)
    for T, D in COMBINE_SHAPES + [INSTANCE_SHAPE]:
        ks += combine_case(T, D)[2]
    for case in exceptional_combines():
        ks += case.lambdas
    ks += flag_combine_case()[2]
    return ks
