"""Cumulative tables for the discrete Gaussian noise share (include/flamingo_hip.h): host Python,
stdlib only.  The library samples from a table and does not build one; this module builds it, and answers the two
questions a caller's privacy accounting asks of it.

* table(sigma, tail): the 2 * tail uint64 thresholds of a discrete Gaussian of parameter sigma truncated to
  |Z| <= tail: table[j] = floor(2^64 * sum_{k=-tail}^{j-tail} w(k) / sum_{k=-tail}^{tail} w(k)), w(k) =
  exp(-k^2 / (2 sigma^2)), i.e. 2^64 P(Z <= j - tail).  The sample of a 64-bit draw u is
  #{j : table[j] <= u} - tail, so P(Z = -tail) = table[0] / 2^64 and P(Z = tail) = 1 - table[-1] / 2^64.
* tail_mass(sigma, tail): the mass the untruncated discrete Gaussian has beyond tail, which goes into the caller's delta.
* moments(table): the exact mean and variance of the law a table samples, as Fractions.
* default_tail(sigma): ceil(10 sigma).

sigma is taken as the exact rational of the Python float passed; everything is computed with `decimal` at 120
significant digits, far beyond the 2^-64 the table resolves.
"""
from __future__ import annotations

import decimal
import math
from fractions import Fraction

import numpy as np

MAX_TAIL = 512          # the library's limit: a table of at most 8 KiB, and 2 * tail <= 1024 for the decode calls
_PREC = 120


def default_tail(sigma: float) -> int:
    """ceil(10 sigma): beyond it the untruncated law has less than 2^-64 of its mass for every sigma >= 0.2."""
    return int(math.ceil(10.0 * float(sigma)))


def _check(sigma: float, tail: int):
    sigma = float(sigma)
    if not (sigma > 0.0) or not math.isfinite(sigma):
        raise ValueError("sigma must be finite and positive")
    if int(tail) != tail or not 1 <= int(tail) <= MAX_TAIL:
        raise ValueError(f"tail must be an integer in 1..{MAX_TAIL}")
    return decimal.Decimal(sigma), int(tail)      # Decimal(float) is exact


def _weights(ctx, sigma: decimal.Decimal, ks):
    two_s2 = ctx.multiply(2, ctx.multiply(sigma, sigma))
    return [ctx.exp(ctx.divide(decimal.Decimal(-k * k), two_s2)) for k in ks]


def table(sigma: float, tail: int) -> np.ndarray:
    """The (2 * tail,) uint64 table of the discrete Gaussian of parameter sigma truncated to |Z| <= tail."""
    sigma, tail = _check(sigma, tail)
    ctx = decimal.Context(prec=_PREC, rounding=decimal.ROUND_HALF_EVEN)
    half = _weights(ctx, sigma, range(tail + 1))                      # w(0) .. w(tail); w(-k) = w(k)
    w = half[:0:-1] + half                                            # k = -tail .. tail
    acc, total = decimal.Decimal(0), decimal.Decimal(0)
    for x in w:                                                       # ctx.add: the + operator rounds to 28 digits
        total = ctx.add(total, x)
    out = np.empty(2 * tail, np.uint64)
    scale = decimal.Decimal(2 ** 64)
    for j in range(2 * tail):
        acc = ctx.add(acc, w[j])
        v = int(ctx.divide(ctx.multiply(acc, scale), total).to_integral_value(rounding=decimal.ROUND_FLOOR))
        out[j] = min(v, 2 ** 64 - 1)
    return out


def tail_mass(sigma: float, tail: int) -> float:
    """P(|Z| > tail) of the untruncated discrete Gaussian of parameter sigma on the integers."""
    sigma = float(sigma)
    if not (sigma > 0.0) or not math.isfinite(sigma) or int(tail) != tail or tail < 0:
        raise ValueError("sigma must be finite and positive, tail a non-negative integer")
    tail = int(tail)
    ctx = decimal.Context(prec=_PREC, rounding=decimal.ROUND_HALF_EVEN, Emin=-10 ** 9, Emax=10 ** 9)
    s = decimal.Decimal(sigma)
    # w(k) < 10^-_PREC w(0) from k^2 > 2 sigma^2 _PREC ln 10 on: nothing beyond changes the sums at this precision
    k_end = max(tail + 1, int(math.sqrt(2.0 * sigma * sigma * _PREC * math.log(10.0))) + 2)
    w = _weights(ctx, s, range(k_end + 1))
    inside, beyond = w[0], decimal.Decimal(0)
    for k in range(1, k_end + 1):
        if k <= tail:
            inside = ctx.add(inside, ctx.multiply(2, w[k]))
        else:
            beyond = ctx.add(beyond, ctx.multiply(2, w[k]))
    return float(ctx.divide(beyond, ctx.add(inside, beyond)))


def pmf(table_) -> list:
    """The law a table samples, exactly: P(Z = c - tail) for c = 0 .. 2 * tail, as Fractions that sum to 1."""
    t = [int(v) for v in np.asarray(table_, dtype=np.uint64)]
    if len(t) < 2 or len(t) % 2 or any(b < a for a, b in zip(t, t[1:])):
        raise ValueError("a table holds 2 * tail non-decreasing uint64 entries")
    edges = [0] + t + [2 ** 64]
    return [Fraction(b - a, 2 ** 64) for a, b in zip(edges, edges[1:])]


def moments(table_):
    """(mean, variance) of the law a table samples, as Fractions."""
    p = pmf(table_)
    tail = (len(p) - 1) // 2
    mean = sum((c - tail) * q for c, q in enumerate(p))
    second = sum((c - tail) ** 2 * q for c, q in enumerate(p))
    return mean, second - mean * mean


def fourth_central_moment(table_) -> Fraction:
    """E (Z - mean)^4 of the law a table samples: what the standard error of a sample variance is made of."""
    p = pmf(table_)
    tail = (len(p) - 1) // 2
    mean = sum((c - tail) * q for c, q in enumerate(p))
    return sum((c - tail - mean) ** 4 * q for c, q in enumerate(p))
