"""Deterministic edge inputs for the tail of hash_to_curve_kernel (flamingo_amd/csrc/flm_p256.hip:
mod_n_384, h2c_map, the lane swap, jac_add and the affine conversion, i.e. h2c_tail) as rows of 96
uniform bytes for flm_h2c_from_uniform, with their expected points from the big-int oracle
(oracle/ec_oracle.h2c_from_uniform).  No test functions: the premises are checked without a GPU by
tests/test_h2c_cases_cpu.py, the kernel against the rows by tests/test_h2c_edges_gpu.py.

A row is two 48-byte big-endian halves; lane 2m of the kernel reduces and maps half 0, lane 2m+1
half 1, and the even lane adds the two points.

* reduction family: 384-bit values for mod_n_384 -- multiples of n and their neighbours, powers of
  two at the limb boundaries, single limbs of ones, values whose low 256 bits overflow on a late
  fold, and one witness for every fold count (tools/h2c_reduce_model.py).  Each sits in one half
  (alternating) beside an ordinary seeded value.
* map family: u < n for h2c_map -- 0 (as 0, as n, as the largest multiple of n), the roots of 1/10
  (den = 0), small and large u, u whose Montgomery form has edge limbs, 64 random u.  Each is
  crossed with one ordinary value in both lane orders.
* pair family: (u0, u1) whose points are equal (jac_add doubles) or opposite (infinity).
* edge_batch(n, rot): n rows with special rows at index 0, n - 1 and on both sides of every
  32-row boundary (a 64-lane workgroup holds 32 rows), ordinary rows elsewhere.
"""
from __future__ import annotations

import functools
import os
import random
import sys
from collections import namedtuple

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _d in ("oracle", "tools"):
    if os.path.join(_ROOT, _d) not in sys.path:
        sys.path.insert(0, os.path.join(_ROOT, _d))

import ec_oracle as E  # noqa: E402
import h2c_reduce_model as M  # noqa: E402

P, N = E.P, E.N
R = 2**256
R_INV = pow(R, -1, P)
NC = R - N                              # kNc
TOP = 2**384
KMAX = (TOP - 1) // N                   # the largest k with k n < 2^384
# both square roots of 1/10 mod p: 100 u^4 - 10 u^2 = 10 u^2 (10 u^2 - 1) = 0
S_PLUS = pow(pow(10, -1, P), (P + 1) // 4, P)
S_MINUS = P - S_PLUS
ROOTS = (S_PLUS, S_MINUS)
B30 = E.B * pow(30, -1, P) % P          # x of map(0) and map(+-sqrt(1/10))

Row = namedtuple("Row", "name ub u0 u1 special")   # special: subset of {"inf", "zero", "den0", "double"}


# ------------------------------------------------------------------ what the oracle's map does
MapTrace = namedtuple("MapTrace", "den0 flip root point")


def map_trace(u: int) -> MapTrace:
    """The branches ec_oracle.map_to_curve takes for u < n: den == 0 (x1 = b/30), the sgn0 flip,
    which candidate gave the root (1: g(x1) is a square, 2: g(x2)), and the point."""
    assert 0 <= u < N
    den = (100 * pow(u, 4, P) - 10 * pow(u, 2, P)) % P
    x1 = B30 if den == 0 else (-E.B * pow(E.A, -1, P)) * (1 + pow(den, -1, P)) % P
    gx1 = (x1 ** 3 + E.A * x1 + E.B) % P
    sq1 = pow(gx1, (P - 1) // 2, P) in (0, 1)
    pt = E.map_to_curve(u)
    return MapTrace(den == 0, (u == 0) != (pt[1] == 0), 1 if sq1 else 2, pt)


def ordinary(k: int) -> int:
    """Seeded 384-bit value number k (an ordinary half: nothing special about it)."""
    return random.Random(7000 + k).getrandbits(384)


def half(v: int) -> bytes:
    assert 0 <= v < TOP
    return v.to_bytes(48, "big")


def make_row(name: str, v0: int, v1: int) -> Row:
    u0, u1 = v0 % N, v1 % N
    q0, q1 = E.map_to_curve(u0), E.map_to_curve(u1)
    special = set()
    if u0 == 0 or u1 == 0:
        special.add("zero")
    if u0 in (0,) + ROOTS or u1 in (0,) + ROOTS:
        special.add("den0")
    if q0 == q1:
        special.add("double")
    if q0 == E.neg(q1):
        special.add("inf")
    return Row(name, half(v0) + half(v1), u0, u1, frozenset(special))


# ------------------------------------------------------------------ reduction family
def _dedup(pairs):
    seen, out = set(), []
    for name, v in pairs:
        if 0 <= v < TOP and v not in seen:
            seen.add(v)
            out.append((name, v))
    return out


@functools.lru_cache(maxsize=None)
def reduction_values() -> list:
    """[(name, v)]: distinct 384-bit inputs of mod_n_384."""
    c = [("0", 0), ("1", 1), ("n-1", N - 1), ("n", N), ("n+1", N + 1), ("2n-1", 2 * N - 1), ("2n", 2 * N),
         ("2^256-1", R - 1), ("2^256", R), ("2^256+1", R + 1)]
    for kn, k in (("2", 2), ("3", 3), ("2^32", 2**32), ("2^64", 2**64), ("2^96", 2**96), ("2^128-1", 2**128 - 1),
                  ("kmax", KMAX)):
        c += [(f"{kn}n{d:+d}", k * N + d) for d in (-1, 0, 1)]
    c += [("2^384-1", TOP - 1), ("2^384-2", TOP - 2)]
    for a in range(0, 384, 32):
        c += [(f"2^{a}", 2**a), (f"2^{a}-1", 2**a - 1), (f"2^384-2^{a}", TOP - 2**a)]
    c += [(f"limb{i}", (2**32 - 1) << (32 * i)) for i in range(12)]
    # lo + hi Nc overflows 2^256 (or just does not) when hi is down to 1: a carry back into limb 8 on a late fold
    for ln, lo in (("2^256-1", R - 1), ("2^256-Nc-1", R - NC - 1), ("2^256-Nc", R - NC), ("2^256-Nc+1", R - NC + 1),
                   ("n-1", N - 1), ("n", N)):
        for hn, hi in (("0", 0), ("1", 1), ("2", 2), ("2^32", 2**32), ("2^64", 2**64), ("2^96", 2**96),
                       ("2^127", 2**127), ("2^128-1", 2**128 - 1)):
            c.append((f"hi={hn},lo={ln}", hi << 256 | lo))
    c += [(f"folds{k}", v) for k, v in sorted(M.FOLD_WITNESSES.items())]
    return _dedup(c)


# ------------------------------------------------------------------ map family
MONT_K = [("1", 1), ("2", 2), ("2^32-1", 2**32 - 1), ("2^32", 2**32), ("2^224", 2**224), ("2^255", 2**255),
          ("p-2", P - 2), ("p-1", P - 1)]
N_RANDOM_U = 64


@functools.lru_cache(maxsize=None)
def map_values() -> list:
    """[(name, v)]: v is the 384-bit value of the half; v mod n is the u that h2c_map sees (v = u but
    for the two other spellings of 0)."""
    c = [("u=0", 0), ("u=0 as n", N), ("u=0 as kmax n", KMAX * N), ("+sqrt(1/10)", S_PLUS), ("-sqrt(1/10)", S_MINUS),
         ("u=1", 1), ("u=2", 2), ("u=n-1", N - 1), ("u=p-n+5", P - N + 5), ("u=n-(p-n+5)", N - (P - N + 5))]
    c += [(f"mont {kn}", k * R_INV % P) for kn, k in MONT_K]      # Montgomery form u R mod p = k
    rng = random.Random(1010)
    c += [(f"random u {i}", rng.randrange(1, N)) for i in range(N_RANDOM_U)]
    return c


def random_us() -> list:
    return [v for name, v in map_values() if name.startswith("random u")]


# ------------------------------------------------------------------ pair family
@functools.lru_cache(maxsize=None)
def doubling_us() -> tuple:
    """Three ordinary u in (p - n, n): p - u is below n too and maps to the same point."""
    rng = random.Random(2020)
    out = []
    while len(out) < 3:
        u = rng.randrange(1, N)
        if P - N < u < N and P - u < N:
            out.append(u)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def pair_values() -> list:
    """[(name, v0, v1, kind)], kind "inf" or "double"."""
    c = []
    for sn, s in (("+s", S_PLUS), ("-s", S_MINUS)):
        c += [(f"(0,{sn})", 0, s, "inf"), (f"({sn},0)", s, 0, "inf")]
    c += [("(0,0)", 0, 0, "double"), ("(+s,+s)", S_PLUS, S_PLUS, "double"), ("(-s,-s)", S_MINUS, S_MINUS, "double"),
          ("(+s,-s)", S_PLUS, S_MINUS, "double"), ("(n,kmax n)", N, KMAX * N, "double")]
    for i, u in enumerate(doubling_us()):
        c += [(f"(u{i},u{i})", u, u, "double"), (f"(u{i},p-u{i})", u, P - u, "double"),
              (f"(p-u{i},u{i})", P - u, u, "double")]
    return c


# ------------------------------------------------------------------ the rows
@functools.lru_cache(maxsize=None)
def rows() -> tuple:
    """Every case as a Row: the reduction values (alternating halves; the fold witnesses in both),
    every map value crossed with one ordinary value in both lane orders, and the pairs."""
    out = []
    for k, (name, v) in enumerate(reduction_values()):
        o = ordinary(k)
        both = v in M.FOLD_WITNESSES.values()
        if both or k % 2 == 0:
            out.append(make_row(f"red {name} | ord", v, o))
        if both or k % 2 == 1:
            out.append(make_row(f"red ord | {name}", o, v))
    for k, (name, v) in enumerate(map_values()):
        o = ordinary(1000 + k)
        out.append(make_row(f"map {name} | ord", v, o))
        out.append(make_row(f"map ord | {name}", o, v))
    for name, v0, v1, _ in pair_values():
        out.append(make_row(f"pair {name}", v0, v1))
    return tuple(out)


def special_rows() -> tuple:
    """The rows with an infinity result, a u = 0 half or a den = 0 half."""
    return tuple(r for r in rows() if r.special & {"inf", "zero", "den0"})


@functools.lru_cache(maxsize=None)
def expect(ub: bytes):
    """ec_oracle.h2c_from_uniform, remembered: (wire bytes, flags word)."""
    pt = E.h2c_from_uniform(ub)
    return E.wire(pt), 4 if pt is None else 0


# ------------------------------------------------------------------ batch edges
BATCH_SIZES = (1, 2, 31, 32, 33, 63, 64, 65, 129)
GROUP_ROWS = 32                          # kEcThreads = 64 lanes, two per row


def edge_positions(n: int) -> list:
    pos = {0, n - 1}
    for b in range(GROUP_ROWS, n + 1, GROUP_ROWS):
        pos |= {b - 1, b} & set(range(n))
    return sorted(pos)


@functools.lru_cache(maxsize=None)
def edge_kinds() -> tuple:
    """An infinity pair, a doubling pair and a row with u = 0 (in the odd lane)."""
    u = doubling_us()[0]
    return (make_row("inf (0,+s)", 0, S_PLUS), make_row("double (u,p-u)", u, P - u),
            make_row("zero (ord,0)", ordinary(5000), 0))


@functools.lru_cache(maxsize=None)
def edge_batch(n: int, rot: int) -> tuple:
    """n rows: the three edge_kinds() in turn (starting at kind `rot`) at edge_positions(n), ordinary
    rows elsewhere.  Over rot = 0, 1, 2 every kind sits at every edge position."""
    kinds = edge_kinds()
    batch = [make_row(f"ord {i}", ordinary(6000 + i), ordinary(6500 + i)) for i in range(n)]
    for j, i in enumerate(edge_positions(n)):
        batch[i] = kinds[(j + rot) % 3]
    return tuple(batch)


@functools.lru_cache(maxsize=None)
def flag_batch() -> tuple:
    """67 rows: infinity rows (the four spellings in turn) at the even indices, ordinary rows between."""
    inf = [make_row(name, v0, v1) for name, v0, v1, kind in pair_values() if kind == "inf"]
    return tuple(inf[(i // 2) % len(inf)] if i % 2 == 0 else make_row(f"ord {i}", ordinary(8000 + i), ordinary(8500 + i))
                 for i in range(67))
