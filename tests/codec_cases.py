"""The fixed-point codec (include/flamingo_hip.h) restated in numpy, and the case lists of
its tests.  No test functions: the premises of the lists are checked without a GPU by tests/test_codec_cpu.py,
the kernels (encode_mask_kernel, decode_sum_kernel) bit for bit against them by tests/test_codec_gpu.py.

* encode / decode / headroom_ok restate the codec; the dither stream is oracle.prg, the reference's PRG.
* value_row(f, c): the edge values of one parameter pair -- signed zeros, subnormals, +-c and the floats
  next to it on both sides, infinities, NaN, the ties of nearest-even.
* threshold_row(): for the fixed dither seed DITHER, a row whose fractions sit one step either side of the
  stochastic threshold at slots where the stream's word is small enough for a float32 to hit it exactly.
* DECODE_WORDS / DECODE_COUNTS: the ring words and counts of the decode cases.
"""
from __future__ import annotations

import hashlib
import math
import os
import sys
from fractions import Fraction

import numpy as np

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if os.path.join(_ROOT, "oracle") not in sys.path:
    sys.path.insert(0, os.path.join(_ROOT, "oracle"))

import oracle  # noqa: E402

DITHER = hashlib.sha256(b"codec dither").digest()
TIES = ((0.5, 0), (1.5, 2), (2.5, 2), (-0.5, 0), (-1.5, -2))      # t -> rint(t), ties to even
PARAMS = ((16, 4.0), (0, 1000.0), (30, 1.0))                       # (frac_bits, clip) of the value rows
DECODE_WORDS = np.array([0, 1, 0xFFFFFFFF, 0x7FFFFFFF, 0x80000000, 2**24 + 1], np.uint32)
DECODE_COUNTS = (1, 3, 4096)
THRESHOLD_L = 2077          # slots scanned for small dither words (about 1 in 256 is below 2^24)
THRESHOLD_F, THRESHOLD_C = 16, 4.0


# ------------------------------------------------------------------ the codec
def encode(x, frac_bits: int, clip: float, dither: bytes | None = None):
    """(ring words uint32, clipped mask bool) of the float32 vector x; dither: 32 bytes = stochastic rounding."""
    x = np.asarray(x, np.float32)
    assert x.ndim == 1
    c = np.float32(clip)
    with np.errstate(invalid="ignore"):
        nan = np.isnan(x)
        clipped = nan | (np.abs(x) > c)
        xc = np.minimum(np.maximum(np.where(nan, np.float32(0), x), -c), c).astype(np.float32)
        t = (xc * np.float32(2.0 ** frac_bits)).astype(np.float32)          # exact: a power of two
    if dither is None:
        q = np.rint(t).astype(np.int64)
    else:
        ti = np.trunc(t)
        fr = np.abs(t - ti).astype(np.float32)                              # exact: a subset of t's bits
        thr = np.trunc(fr.astype(np.float64) * 2.0 ** 32).astype(np.uint64)
        assert np.all(thr < 2 ** 32)
        r = oracle.prg(dither, x.shape[0]).astype(np.uint64)
        q = ti.astype(np.int64) + np.sign(t).astype(np.int64) * (r < thr)
    return (q & 0xFFFFFFFF).astype(np.uint32), clipped


def decode(s, frac_bits: int, count: int = 1) -> np.ndarray:
    """float32(float64(int32(s)) / (float64(count) 2^f)): one double division, one rounding."""
    s = np.ascontiguousarray(s, np.uint32)
    return (s.view(np.int32).astype(np.float64) / (np.float64(count) * 2.0 ** frac_bits)).astype(np.float32)


def headroom_ok(frac_bits: int, clip: float, n: int) -> bool:
    """n ceil(c 2^f) <= 2^31 - 1, in exact integers."""
    return n * math.ceil(Fraction(float(np.float32(clip))) * 2 ** frac_bits) <= 2 ** 31 - 1


def masked(x, frac_bits, clip, seeds, signs, dither=None):
    """encode(x) + sum_k signs[k] PRG(seeds[k]) mod 2^32 -> (row, number of clipped elements)."""
    w, cl = encode(x, frac_bits, clip, dither)
    acc = w.astype(np.uint64)
    for sd, sg in zip(seeds, signs):
        p = oracle.prg(bytes(sd), len(w)).astype(np.uint64)
        acc = acc + p if sg > 0 else acc + (2 ** 32 - p)
    return (acc & 0xFFFFFFFF).astype(np.uint32), int(cl.sum())


# ------------------------------------------------------------------ case lists
def value_row(frac_bits: int, clip: float) -> np.ndarray:
    c = np.float32(clip)
    inf = np.float32(np.inf)
    inside, outside = np.nextafter(c, np.float32(0)), np.nextafter(c, inf)
    v = [0.0, -0.0, 1e-45, -1e-45, 1e-39, -1e-39, 1.1754942e-38, -1.1754942e-38,
         c, -c, inside, -inside, outside, -outside, inf, -inf, np.nan, 3.0e38, -3.0e38]
    step = 2.0 ** -frac_bits
    v += [t * step for t, _ in TIES]
    v += [t * step for t in (0.25, 0.75, -0.25, -0.75, 1.0, -1.0, 3.5, -3.5, 1.4999999, 2.5000002)]
    return np.array(v, np.float32)


def random_row(L: int, clip: float, seed: int, wild: bool = False) -> np.ndarray:
    """L floats, most inside +-clip; wild: a few beyond it, infinities and NaNs as well."""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal(L) * (clip / 3.0)).astype(np.float32)
    if wild and L >= 4:
        idx = rng.choice(L, size=max(1, L // 16), replace=False)
        x[idx] = rng.choice(np.array([np.nan, np.inf, -np.inf, 2 * clip, -3 * clip], np.float32), size=idx.size)
    return x


def threshold_slots():
    """[(slot, r)] of DITHER's stream with 0 < r < 2^24: there (r + 1) 2^-32 and r 2^-32 are float32 values."""
    r = oracle.prg(DITHER, THRESHOLD_L)
    return [(int(l), int(r[l])) for l in np.nonzero((r < 2 ** 24) & (r > 0))[0]]


def threshold_row():
    """(x, [(slot, r, thr, away)]): |t| = thr 2^-32 at the slots of threshold_slots(), thr = r + 1 (the word is
    just below the threshold: rounds away from zero) and thr = r (it is not: truncates) in turn, both signs;
    the other slots hold fractions of all sizes."""
    rng = np.random.default_rng(2077)
    x = (rng.random(THRESHOLD_L) * 6.0 - 3.0).astype(np.float32)
    picks = []
    for n, (l, r) in enumerate(threshold_slots()):
        away = n % 2 == 0
        thr = r + 1 if away else r
        sign = -1.0 if (n // 2) % 2 else 1.0
        x[l] = np.float32(sign * thr * 2.0 ** -32 * 2.0 ** -THRESHOLD_F)
        picks.append((l, r, thr, away))
    return x, picks
