"""The L2 clip of float updates (include/flamingo_hip.h) restated in numpy, and the case lists of
its tests.  No test functions: the premises are checked without a GPU by tests/test_l2_cpu.py, the kernels
(l2_sumsq_kernel, l2_factor_kernel, scale_rows_kernel, rotate_kernel<false, PHASES, true>) bit for bit against them by
tests/test_l2_gpu.py.

* sumsq / factor / clip restate the rule: the float64 sum of the squares in the normative order (tiles of 4096, 16
  consecutive parameters per thread, xor-butterflies over runs of 64 threads, ((w0 + w1) + w2) + w3, then partials
  k, k + 64, ... per lane and the butterflies again), the float32 factor, the float32 multiply.
* clip_forward: the clip composed with rotate_cases.forward, which is what the fused kernel must give: a sign flip
  commutes exactly with a multiply.
* sequential_sumsq: the plain left-to-right float64 sum, the wrong order the ORDER rows tell apart.
* row_with_sumsq: a float32 row whose squares sum to a chosen double exactly, in any order; the edge rows and the
  square-root pins are built with it.
"""
from __future__ import annotations

import math

import numpy as np

import rotate_cases as R

TILE = 4096
LENGTHS = (1, 15, 16, 17, 4095, 4096, 4097, 8193, 64 * 4096 + 5)    # the last: a lane of the row sum holds two partials
BOUND = 1.0 + 2.0 ** -22                                             # ||clip(x)||_2 <= C BOUND
_LANES = np.arange(64)


def _butterflies(a: np.ndarray) -> np.ndarray:
    """a[..., 64] -> the same shape, every lane a + a[lane ^ off] for off = 1, 2, 4, 8, 16, 32 in turn."""
    for off in (1, 2, 4, 8, 16, 32):
        a = a + a[..., _LANES ^ off]
    return a


def squares(x) -> np.ndarray:
    """float64 squares of one row, a non-finite element counting as +0.0; exact."""
    x = np.asarray(x, np.float32)
    assert x.ndim == 1 and len(x) > 0
    d = np.where(np.isfinite(x), x, np.float32(0.0)).astype(np.float64)
    return d * d


def tile_partials(x) -> np.ndarray:
    """The partial of every 4096-parameter tile of the row: what l2_sumsq_kernel stores."""
    sq = squares(x)
    tiles = -(-len(sq) // TILE)
    p = np.zeros(tiles * TILE, np.float64)                       # parameters >= L count as +0.0
    p[:len(sq)] = sq
    p = p.reshape(tiles, 256, 16)
    a = np.zeros((tiles, 256), np.float64)
    for j in range(16):                                          # a thread's 16 squares onto +0.0 in index order
        a = a + p[:, :, j]
    w = _butterflies(a.reshape(tiles, 4, 64))
    assert all(np.array_equal(w[..., 0].view(np.uint64), w[..., k].view(np.uint64)) for k in (1, 31, 63))
    w = w[..., 0]
    return ((w[:, 0] + w[:, 1]) + w[:, 2]) + w[:, 3]


def sumsq(x) -> np.float64:
    """S of one row, in the normative order."""
    t = tile_partials(x)
    p = np.zeros(-(-len(t) // 64) * 64, np.float64)
    p[:len(t)] = t
    acc = np.zeros(64, np.float64)
    for r in p.reshape(-1, 64):                                  # lane k: partials k, k + 64, ... onto +0.0
        acc = acc + r
    return np.float64(_butterflies(acc)[0])


def sequential_sumsq(x) -> np.float64:
    """The squares added left to right: not the rule."""
    acc = np.float64(0.0)
    for v in squares(x):
        acc = acc + v
    return acc


def factor(S, C) -> np.float32:
    C = np.float64(np.float32(C))
    S = np.float64(S)
    if S <= C * C:
        return np.float32(1.0)
    return np.float32(C / np.sqrt(S))                            # IEEE double sqrt and divide, one rounding to float32


def clip(x, C):
    """(x s as float32, s, S) of one row."""
    x = np.asarray(x, np.float32)
    S = sumsq(x)
    s = factor(S, C)
    with np.errstate(invalid="ignore", under="ignore"):
        return (x * s).astype(np.float32), s, S


def clip_forward(x, C, key: bytes, h: int):
    """(rotated floats, non-finite count, s, S): the clip, then rotate_cases.forward."""
    y, s, S = clip(x, C)
    out, bad = R.forward(y, key, h)
    return out, bad, s, S


# ------------------------------------------------------------------ rows with a chosen sum of squares
def row_with_sumsq(n: int, e: int, length: int | None = None) -> np.ndarray:
    """A float32 row whose squares sum to n 4^e exactly, 0 < n < 2^53: integers a_i < 2^24 with sum a_i^2 = n, times
    2^e.  Every partial sum of the squares is an integer below 2^53 times 4^e, so any order of adding gives S exactly."""
    assert 0 < n < 2 ** 53
    terms, rem = [], n
    while rem:
        a = min(math.isqrt(rem), 2 ** 24 - 1)
        terms.append(a)
        rem -= a * a
    x = np.ldexp(np.array(terms, np.float64), e).astype(np.float32)
    assert np.array_equal(x.astype(np.float64), np.ldexp(np.array(terms, np.float64), e))
    if length is not None:
        assert len(x) <= length
        x = np.concatenate([x, np.zeros(length - len(x), np.float32)])
    return x


def double_of(n: int, e: int) -> np.float64:
    return np.float64(math.ldexp(n, 2 * e))


# ------------------------------------------------------------------ case lists
def rows(N: int, L: int, seed: int, C: float) -> np.ndarray:
    """N rows of L finite floats of mixed magnitude: row 0 scaled to a norm of about C / 2, row 1 to 3 C, the rest
    as they come."""
    x = R.rows(N, L, seed)
    for i, target in ((0, 0.5 * C), (1, 3.0 * C)):
        if i < N:
            n = float(np.sqrt(squares(x[i]).sum()))
            if n > 0:
                x[i] = (x[i].astype(np.float64) * (target / n)).astype(np.float32)
    return x


SPECIAL_L = 8193


def order_rows() -> np.ndarray:
    """Rows of SPECIAL_L floats mixing 1e8 and 1: 1e16 + 1 is 1e16 in float64, so a left-to-right sum loses every
    one behind the large element, and the normative order keeps those of the other threads."""
    a = np.ones((4, SPECIAL_L), np.float32)
    a[0, 0] = 1e8
    a[1, 5000] = 1e8
    a[2, 50], a[2, 100:] = 1e8, 0.0                              # one wave of one tile
    a[3, ::1000] = 1e8                                           # several large elements, several tiles
    a[3, 1::2] = 3.0
    return a


def _pad(v) -> np.ndarray:
    out = np.zeros(SPECIAL_L, np.float32)
    out[:len(v)] = v
    return out


def special_batches():
    """[(C, rows (n, SPECIAL_L), names)]: the factor's edges.  At C = 5: S = 0; S = 25 exactly, as (3, 4) and as 25
    equal squares; S one float64 ulp (2^-48) above and below 25; -0.0 and subnormals in a row within the norm; the
    ORDER rows (far outside).  At C = 1: rows of 3.4e38 (S about 4.7e80, a subnormal factor).  At C = 1e-40: rows of
    float32 subnormals, inside and outside the norm."""
    tiny = np.array([1e-45, -3e-45, 1e-39, -0.0, 0.0, 1.0], np.float32)
    five = [(_pad([]), "zero"), (_pad([3.0, 4.0]), "3-4-5"), (row_with_sumsq(25 << 48, -24, SPECIAL_L), "25 exactly"),
            (row_with_sumsq((25 << 48) + 1, -24, SPECIAL_L), "one ulp above"),
            (row_with_sumsq((25 << 48) - 1, -24, SPECIAL_L), "one ulp below"), (_pad(tiny), "tiny within")]
    five += [(r, "order %d" % i) for i, r in enumerate(order_rows())]
    huge = np.full(SPECIAL_L, 3.4e38, np.float32)
    huge[4096:] = 0.0
    mixed = huge.copy()
    mixed[::2] *= np.float32(-1.0)
    sub = np.full(SPECIAL_L, 1e-45, np.float32)
    sub5 = _pad(np.full(5, 1e-45, np.float32))
    return [(5.0, np.stack([r for r, _ in five]), [n for _, n in five]),
            (1.0, np.stack([huge, mixed]), ["4096 of 3.4e38", "alternating signs"]),
            (1e-40, np.stack([sub, sub5, _pad(np.array([1e-39, -1e-39, 1e-39], np.float32)),
                              np.full(SPECIAL_L, 2e-42, np.float32)]),
             ["8193 least subnormals", "5 least subnormals", "three subnormals outside", "8193 subnormals outside"])]


def _odd_root(r: int, bits: int) -> int:
    """x with x^2 = r mod 2^bits, r = 1 mod 8 (Hensel: one bit at a time)."""
    x = 1
    for k in range(3, bits):
        if (x * x - r) >> k & 1:
            x += 1 << (k - 1)
    assert (x * x - r) % (1 << bits) == 0
    return x


def sqrt_pins():
    """[(n, e)]: S = n 4^e whose square root a wrong last bit would show -- perfect squares, their float64
    neighbours, and S whose exact root lies within 2^-90 (relative) of half-way between two doubles, from either side:
    1 + (2 k + 1) 2^-52 (root just below 1 + (2 k + 1) 2^-53), and the doubles just above ((2 Y + 1) 2^-53)^2 for
    the 2 Y + 1 whose square is -7, -15, -23 mod 2^54.  Each at three scales."""
    pins = []
    for y in (3, 5, 2 ** 24 - 1, 94906265, 2 ** 26 + 1):          # y^2 < 2^53
        pins += [y * y, y * y + 1, y * y - 1]
    pins += [2 ** 52 + 2 * k + 1 for k in range(4)]
    for small in (7, 15, 23):
        r = _odd_root(2 ** 54 - small, 54)
        for x in (r, 2 ** 54 - r, (r + 2 ** 53) % 2 ** 54, (2 ** 54 - r + 2 ** 53) % 2 ** 54):
            if not 2 ** 53 <= x < 2 ** 54:
                continue
            n = (x * x + small) >> 54                             # (x 2^-53)^2 = (n - small 2^-54) 2^-52
            if n < 2 ** 53:                                       # S in [1, 2): a 53-bit n
                pins.append(n)
            elif n % 4 == 0:                                      # S in [2, 4): n / 4 at the next scale up
                pins.append(n // 4)
    return [(n, e) for n in pins for e in (-26, 0, -60)]
