"""Conditional stochastic rounding (include/flamingo_hip.h) restated in numpy and Python integers,
and the case lists of its tests.  No test functions: the premises are checked without a GPU by tests/test_round_cpu.py,
the kernels (round_sumsq_kernel, round_select_kernel) bit for bit against them by tests/test_round_gpu.py.

* q / sumsq restate the rule: the integers the codec's stochastic encode (codec_cases.encode) rounds a row to under a
  dither seed, as int32, and the sum of their squares as a Python integer.
* select: the first candidate within the bound, or A.
* bound: flm_round_bound's float64 sequence, operation by operation; bound_exact the same formula in Fractions.
* cases(): (name, frac_bits, clip, row, candidates) -- the codec's value rows, the threshold row with DITHER among its
  candidates, wild random rows at every length of l2_cases.LENGTHS.
"""
from __future__ import annotations

import hashlib
import math
from fractions import Fraction

import numpy as np

import codec_cases as CC
import l2_cases as l2

LENGTHS = l2.LENGTHS
ATTEMPTS = (1, 3, 8)
WRAP_GUARD = (30, 1.0, np.array([1.0, -1.0, 1.0], np.float32), 3 * 2 ** 60)      # (f, c, x, Q under any seed)
SLACK = 1.0 + 2.0 ** -19
# the (d, s = C 2^f) points of the issue's simulation, as (C, f, d)
SIMULATED = ((2.28125, 7, 4096), (2.28125, 7, 65536), (1.0, 4, 65536), (36.5, 0, 1024))


def seed(tag: str, i: int = 0) -> bytes:
    return hashlib.sha256(f"round {tag} {i}".encode()).digest()


def candidates(tag: str, N: int, A: int) -> np.ndarray:
    """(N, A, 32) uint8: candidate a of row i is seed(tag, i * A + a)."""
    return np.frombuffer(b"".join(seed(tag, k) for k in range(N * A)), np.uint8).reshape(N, A, 32).copy()


# ------------------------------------------------------------------ the rule
def q(x, frac_bits: int, clip: float, dither: bytes) -> np.ndarray:
    """int32 q_l of the row under the dither seed: the codec's stochastic encode, reinterpreted."""
    words, _ = CC.encode(x, frac_bits, clip, bytes(dither))
    return words.view(np.int32)


def sumsq(x, frac_bits: int, clip: float, dither: bytes) -> int:
    """Q(seed) = sum q_l^2, a Python integer."""
    return sum(v * v for v in q(x, frac_bits, clip, dither).tolist())


def sums(xs, frac_bits: int, clip: float, cands) -> list:
    """[[Q(candidate a of row i)]]"""
    return [[sumsq(x, frac_bits, clip, bytes(c)) for c in row] for x, row in zip(xs, cands)]


def select(Q, max_sumsq: int) -> int:
    """The smallest a with Q[a] <= max_sumsq, else len(Q)."""
    return next((a for a, v in enumerate(Q) if v <= max_sumsq), len(Q))


def bound(C, frac_bits: int, d: int, tail: float) -> int:
    """flm_round_bound in numpy float64, one rounding per operation, in the header's order."""
    s = (np.float64(np.float32(C)) * np.float64(2.0 ** frac_bits)) * np.float64(SLACK)
    r = np.sqrt(np.float64(d))
    b1 = (s + r) * (s + r)
    b2 = (s * s + np.float64(d) * np.float64(0.25)) + np.float64(tail) * (s + r * np.float64(0.5))
    return int(np.floor(min(b1, b2)))


def bound_branch(C, frac_bits: int, d: int, tail: float) -> int:
    """1 when (s + sqrt(d))^2 is the smaller, 2 when the tail bound is."""
    s = (np.float64(np.float32(C)) * np.float64(2.0 ** frac_bits)) * np.float64(SLACK)
    r = np.sqrt(np.float64(d))
    return 1 if (s + r) * (s + r) <= (s * s + np.float64(d) * 0.25) + np.float64(tail) * (s + r * 0.5) else 2


def tail_of(beta: float) -> float:
    return math.sqrt(2.0 * math.log(1.0 / beta))


BOUND_GRID = [(C, f, d, k) for (C, f, d) in SIMULATED for k in (0.0, 1.0, tail_of(0.1), 40.0, 1e6)] + \
    [(1.0, 0, 1, 0.0), (1.0, 30, 3, 1.0), (1e-3, 0, 2 ** 36, 1.0), (1.9, 30, 2 ** 20, 0.3), (0.5, 16, 4097, 2.5),
     (2.28125, 7, 4032, 1.0)]


# ------------------------------------------------------------------ case lists
def max_len(frac_bits: int, clip: float) -> int:
    """The longest row flm_round_check takes at (f, c): floor((2^64 - 1) / B^2), B = ceil(c 2^f), and 2^36."""
    B = math.ceil(Fraction(float(np.float32(clip))) * 2 ** frac_bits)
    return min((2 ** 64 - 1) // (B * B), 2 ** 36)


def threshold_case():
    """The codec's threshold row, and candidates with DITHER at index 1: under DITHER the picked slots sit one step
    either side of the threshold, under any other seed they do not."""
    x, picks = CC.threshold_row()
    cands = np.stack([np.frombuffer(s, np.uint8) for s in (seed("threshold", 0), CC.DITHER, seed("threshold", 2))])
    return x, picks, cands


def cases():
    """[(name, frac_bits, clip, x (L,), candidates (8, 32))]"""
    out = []
    for f, c in CC.PARAMS:
        # the call's rule L B^2 <= 2^64 - 1 allows 15 parameters at (30, 1.0): that value row goes in pieces
        row, most = CC.value_row(f, c), max_len(f, c)
        for k in range(0, len(row), most):
            out.append((f"values f={f} from {k}", f, c, row[k:k + most], candidates(f"values {f} {k}", 1, 8)[0]))
    x, _, cands = threshold_case()
    more = candidates("threshold more", 1, 5)[0]
    out.append(("threshold", CC.THRESHOLD_F, CC.THRESHOLD_C, x, np.concatenate([cands, more])))
    return out


def random_rows(N: int, L: int, clip: float, tag: int) -> np.ndarray:
    """N wild rows of L floats: most inside +-clip, some beyond, infinities and NaNs."""
    return np.stack([CC.random_row(L, clip, 7000 + 31 * tag + i, wild=True) for i in range(N)])
