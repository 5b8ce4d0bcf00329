"""Deterministic edge inputs for the Feldman share check (feldman_verify_kernel in
flamingo_amd/csrc/flm_p256.hip, crypto.feldman_verify) and their expected results from the big-int
oracle (oracle/ec_oracle.py).  No test functions: the premises are checked without a GPU by
tests/test_feldman_cases_cpu.py, the kernel against them by tests/test_feldman_gpu.py.  These are the
inputs no honest key generation reaches; the honest ones are the reference's own, in
tests/golden/dkg_golden.json.

* expected() evaluates a row the reference's way (agent/dkg/SA_ClientAgent.py:219-228): the sum of
  C_k times the unreduced integer x ** k, not Horner's rule, so the kernel's schedule is checked
  against another one.
* horner_events() restates the kernel's schedule over the exponents (every commitment here is c_k G
  with c_k known) and says where an addition meets an operand at infinity, P + P or P - P.
* CASES: the case list; every case carries its claimed verdict and flags, which the CPU test holds
  to expected().
* pool(): the cases padded to one T with infinity as top terms (a zero coefficient), for the
  batch-shape tests.
"""
from __future__ import annotations

import functools
import os
import random
import sys
from collections import namedtuple

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if os.path.join(_ROOT, "oracle") not in sys.path:
    sys.path.insert(0, os.path.join(_ROOT, "oracle"))

import ec_oracle as E  # noqa: E402

P, N = E.P, E.N
INF = bytes(64)
X_MAX = (1 << 32) - 1
TOP = (1 << 256) - 1
F_SHARE, F_COMMIT, F_INF, F_XBITS = 1, 2, 4, 8      # flags bits 0..3

# name; com: T wire commitments (64 bytes each); coeffs: their exponents, or None where a commitment
# is not c G; x, x_bits, share: the row; ok, flags: the claimed result
Case = namedtuple("Case", "name com coeffs x x_bits share ok flags")


@functools.lru_cache(maxsize=None)
def mulg(k: int):
    return E.mul(k % N)


def commit(coeffs) -> list:
    return [E.wire(mulg(c)) for c in coeffs]


def poly(coeffs, x: int) -> int:
    return sum(c * pow(x, k, N) for k, c in enumerate(coeffs)) % N


def unwire(b: bytes):
    """A wire commitment as the check sees it: (point or None, valid).  64 zero bytes are infinity and
    valid; a coordinate >= p or a point off the curve is invalid and counts as infinity."""
    if b == INF:
        return None, True
    pt = (int.from_bytes(b[:32], "big"), int.from_bytes(b[32:], "big"))
    if pt[0] >= P or pt[1] >= P or not E.on_curve(pt):
        return None, False
    return pt, True


@functools.lru_cache(maxsize=None)
def _power_sum(com: tuple, x: int):
    acc, valid = None, True
    for k, b in enumerate(com):
        pt, ok = unwire(b)
        valid = valid and ok
        if pt is not None:
            acc = E.add(acc, E.mul(x ** k, pt) if x or k == 0 else None)
    return acc, valid


def expected(com, x: int, x_bits: int, share: int):
    """(ok, flags, wire point of F) of one row, by the reference's sum of C_k * (x ** k)."""
    flags = 0
    if x >> x_bits:
        flags |= F_XBITS
    f, valid = _power_sum(tuple(com), x & ((1 << x_bits) - 1))
    if not valid:
        flags |= F_COMMIT
    if f is None:
        flags |= F_INF
    if share >= N:
        flags |= F_SHARE
    ok = flags in (0, F_INF) and mulg(share) == f
    return ok, flags, E.wire(f)


def horner_events(coeffs, x: int, x_bits: int) -> list:
    """The kernel's right-hand side over exponents mod n: acc = c[T-1]; for k = T-2 .. 0:
    R = 0; for each of the x_bits bits of x from the top: R = 2 R, and R = R + acc where the bit is
    set; acc = R + c[k].  Returns [(k, where, kind)] for every addition that is exceptional: where is
    a bit index or "term", kind "inf" (an operand at infinity), "double" (P + P) or "cancel" (P - P)."""
    def kind(a, b):
        if a == 0 or b == 0:
            return "inf"
        if a == b:
            return "double"
        if (a + b) % N == 0:
            return "cancel"
        return None
    ev = []
    acc = coeffs[-1] % N
    for k in range(len(coeffs) - 2, -1, -1):
        r = 0
        for b in range(x_bits - 1, -1, -1):
            r = 2 * r % N
            if (x >> b) & 1:
                if kind(r, acc):
                    ev.append((k, b, kind(r, acc)))
                r = (r + acc) % N
        c = coeffs[k] % N
        if kind(r, c):
            ev.append((k, "term", kind(r, c)))
        acc = (r + c) % N
    return ev


def _flip_y(b: bytes) -> bytes:
    return b[:63] + bytes([b[63] ^ 1])


def _cases() -> list:
    rnd = random.Random("feldman-cases")
    rs = lambda: rnd.randrange(1, N)  # noqa: E731
    out = []

    def add(name, coeffs, x, x_bits, share, ok, flags, com=None):
        out.append(Case(name, com if com is not None else commit(coeffs), list(coeffs) if com is None else None,
                        x, x_bits, share, ok, flags))

    # a constant polynomial at several x (T = 1: no Horner step at all)
    c = rs()
    for x in (0, 1, 5, 63):
        add(f"const_x{x}", [c], x, 6, c, True, 0)
    add("const_wrong", [c], 5, 6, (c + 1) % N, False, 0)
    # x = 0: the secret against C_0, whatever the higher terms
    co = [rs(), rs(), rs()]
    add("x0", co, 0, 6, co[0], True, 0)
    add("x0_wrong", co, 0, 6, poly(co, 1), False, 0)
    # x = 2^32 - 1 under x_bits = 32
    add("x_max", co, X_MAX, 32, poly(co, X_MAX), True, 0)
    add("x_max_wrong", co, X_MAX, 32, poly(co, X_MAX - 1), False, 0)
    # F(x) at infinity with share 0: accepted, flag bit 2 (the last addition is P - P)
    c1 = rs()
    add("f_inf_share0", [-37 * c1 % N, c1], 37, 6, 0, True, F_INF)
    add("f_inf_share1", [-37 * c1 % N, c1], 37, 6, 1, False, F_INF)
    # the last addition is a doubling: c0 = x c1
    add("final_double", [37 * c1 % N, c1], 37, 6, 74 * c1 % N, True, 0)
    # acc passes through infinity in the middle: c1 = -x c2, so F(x) = C_0
    c2, c0 = rs(), rs()
    add("mid_inf", [c0, -41 * c2 % N, c2], 41, 6, c0, True, 0)
    # an infinity commitment as top, middle and constant term; all of them
    a, b = rs(), rs()
    add("inf_top", [a, b, 0], 9, 6, poly([a, b, 0], 9), True, 0)
    add("inf_mid", [a, 0, b], 9, 6, poly([a, 0, b], 9), True, 0)
    add("inf_const", [0, a, b], 9, 6, poly([0, a, b], 9), True, 0)
    add("all_inf_share0", [0, 0, 0], 9, 6, 0, True, F_INF)
    add("all_inf_share1", [0, 0, 0], 9, 6, 1, False, F_INF)
    # share values: f(x) = s exactly, for small s, the top bit and the top of the range
    for label, s in (("1", 1), ("2", 2), ("3", 3), ("15", 15), ("16", 16), ("17", 17), ("2p255", 1 << 255),
                     ("n_minus_2", N - 2), ("n_minus_1", N - 1)):
        c1 = rs()
        add(f"share_{label}", [(s - 11 * c1) % N, c1], 11, 6, s, True, 0)
    # shares >= n are refused, not reduced: each would pass reduced mod n
    # (n itself: f(x) = 0, so F is at infinity as well)
    for label, s in (("n", N), ("n_plus_1", N + 1), ("2p256_minus_1", TOP)):
        c1 = rs()
        add(f"share_{label}", [(s - 11 * c1) % N, c1], 11, 6, s, False, F_SHARE | (F_INF if s == N else 0))
    # commitments that are no points: a flipped y bit, a coordinate = p (the row fails, flag bit 1)
    co = [rs(), rs(), rs()]
    good = commit(co)
    s = poly(co, 13)
    for k in range(3):
        bad = list(good)
        bad[k] = _flip_y(good[k])
        add(f"flip_y_term{k}", co, 13, 6, s, False, F_COMMIT, com=bad)
    px = list(good)
    px[1] = P.to_bytes(32, "big") + good[1][32:]
    add("x_is_p", co, 13, 6, s, False, F_COMMIT, com=px)
    py = list(good)
    py[0] = good[0][:32] + P.to_bytes(32, "big")
    add("y_is_p", co, 13, 6, s, False, F_COMMIT, com=py)
    # x >= 2^x_bits: refused (flag bit 3), although the share is right for the whole x
    add("x_over_bits", co, 64 + 13, 6, poly(co, 64 + 13), False, F_XBITS)
    add("x_over_bits_low_ok", co, 64 + 13, 6, s, False, F_XBITS)
    add("x_at_bits_edge", co, 63, 6, poly(co, 63), True, 0)
    return out


CASES = _cases()
BY_NAME = {c.name: c for c in CASES}


def groups() -> dict:
    """(T, x_bits) -> the cases of that shape: one launch each, dealer i = case i."""
    g = {}
    for c in CASES:
        g.setdefault((len(c.com), c.x_bits), []).append(c)
    return g


POOL_T = 3


@functools.lru_cache(maxsize=None)
def pool() -> tuple:
    """Every case whose x fits its x_bits, padded to POOL_T terms with infinity on top and taken
    under x_bits = 32, valid and invalid rows alternating: (rows, results) with rows
    [(com, x, share)] and results [(ok, flags, point)] from expected()."""
    fit = [c for c in CASES if not c.x >> c.x_bits]
    good, bad = [c for c in fit if c.ok], [c for c in fit if not c.ok]
    order = []
    for i in range(max(len(good), len(bad))):
        order.append(good[i % len(good)])
        order.append(bad[i % len(bad)])
    rows = [(tuple(c.com) + (INF,) * (POOL_T - len(c.com)), c.x, c.share) for c in order]
    return tuple(rows), tuple(expected(com, x, 32, s) for com, x, s in rows)
