"""The packed fixed-point codec (include/flamingo_hip.h) restated in numpy on top of
tests/codec_cases.py, and the case lists of its tests.  No test functions: the premises of the lists are checked
without a GPU by tests/test_pack_cpu.py, the kernels (encode_mask_kernel at P = 2, 4, decode_unpack_kernel) bit for bit
against them by tests/test_pack_gpu.py.

* bias / headroom_ok / encode_packed / decode_packed / masked_packed restate the codec: P = 2 or 4 fields of
  W = 32 / P bits per ring word, field = codec_cases.encode's q + B, B = ceil(c 2^f); the dither stream is
  indexed by parameter; fields of parameters past L hold 0; masks are whole words indexed by word.
* HEADROOM_EDGES: (f, c, P, the largest n with headroom).
* WORST_ROUNDS: (f, c, P, n, L) of the whole rounds at the worst case; worst_inputs makes their clients.
* rotated_value_rows: codec_cases.value_row rotated so every edge value lands in every field.
* threshold_row: codec_cases.threshold_row's construction at (f = 7, c = 1), which the packed widths admit.
* DECODE_WORDS / decode_counts: the summed words and counts of the decode cases.
"""
from __future__ import annotations

import math
from fractions import Fraction

import numpy as np

import codec_cases as K
from codec_cases import oracle

PACKS = (2, 4)
HEADROOM_EDGES = ((7, 1.0, 2, 255), (4, 1.0, 2, 2047), (2, 1.0, 4, 31), (0, 1.0, 4, 127))
WORST_ROUNDS = ((7, 1.0, 2, 255, 2077), (2, 1.0, 4, 31, 2077), (4, 1.0, 2, 1024, 1025), (0, 1.0, 4, 127, 1023))
GPU_ROUNDS = WORST_ROUNDS[:2]
VALUE_PARAMS = ((7, 1.0), (2, 1.0))           # (f, c) of the value rows: (7, 1) fits P = 2, (2, 1) fits both
# adjacent fields at 0 and at 2^W - 1, for either width
DECODE_WORDS = np.array([0xFFFF0000, 0x0000FFFF, 0xFF00FF00, 0x00FF00FF, 0xFFFFFFFF, 0], np.uint32)
THRESHOLD_F, THRESHOLD_C = 7, 1.0
DITHER = K.DITHER


def pack_params(pack: int):
    """(f, c) at which the GPU tests run a width: P = 2 at (7, 1), n <= 255; P = 4 at (2, 1), n <= 31."""
    return {2: (7, 1.0), 4: (2, 1.0)}[pack]


def decode_counts(pack: int):
    return (1, 3, {2: 255, 4: 31}[pack])


def shapes(pack: int):
    P = pack
    return (1, P - 1, P, P + 1, 16 * P - 1, 16 * P, 16 * P + 1, 1024 * P - 1, 1024 * P, 1024 * P + 1, 2077 * P + P - 1)


# ------------------------------------------------------------------ the codec
def bias(frac_bits: int, clip: float) -> int:
    """B = ceil(c 2^f), in exact integers."""
    return math.ceil(Fraction(float(np.float32(clip))) * 2 ** frac_bits)


def headroom_ok(frac_bits: int, clip: float, pack: int, n: int) -> bool:
    """n 2B <= 2^W - 1: no field of a sum over n contributors carries into its neighbour."""
    return n * 2 * bias(frac_bits, clip) <= 2 ** (32 // pack) - 1


def fields(x, frac_bits: int, clip: float, dither: bytes | None = None):
    """(u = q + B per parameter as int64, clipped mask); q is codec_cases.encode's, its dither word PRG(dither)[l]."""
    w, clipped = K.encode(x, frac_bits, clip, dither)
    return w.view(np.int32).astype(np.int64) + bias(frac_bits, clip), clipped


def pack_fields(u, pack: int) -> np.ndarray:
    """word l' = sum_j u[P l' + j] << (W j); fields past len(u) hold 0."""
    u = np.asarray(u, np.int64)
    W, Lw = 32 // pack, -(-len(u) // pack)
    full = np.zeros(Lw * pack, np.int64)
    full[:len(u)] = u
    assert np.all((full >= 0) & (full < 2 ** W))
    return (full.reshape(Lw, pack) << (W * np.arange(pack, dtype=np.int64))).sum(axis=1).astype(np.uint32)


def encode_packed(x, frac_bits: int, clip: float, pack: int, dither: bytes | None = None):
    """(ceil(L / P) ring words uint32, clipped mask bool over the L parameters)."""
    u, clipped = fields(x, frac_bits, clip, dither)
    return pack_fields(u, pack), clipped


def decode_packed(S, L: int, frac_bits: int, clip: float, pack: int, count: int = 1) -> np.ndarray:
    """out[P l' + j] = float32(float64(s_j - count B) / (float64(count) 2^f)), s_j = (S >> W j) & (2^W - 1)."""
    S = np.ascontiguousarray(S, np.uint32).astype(np.int64)
    W = 32 // pack
    assert len(S) == -(-L // pack)
    s = (S[:, None] >> (W * np.arange(pack, dtype=np.int64))) & (2 ** W - 1)
    v = (s.reshape(-1)[:L] - count * bias(frac_bits, clip)).astype(np.float64)
    return (v / (np.float64(count) * 2.0 ** frac_bits)).astype(np.float32)


def masked_packed(x, frac_bits, clip, pack, seeds, signs, dither=None):
    """encode_packed(x) + sum_k signs[k] PRG(seeds[k]) mod 2^32 over the words -> (row, clipped elements)."""
    w, cl = encode_packed(x, frac_bits, clip, pack, dither)
    acc = w.astype(np.uint64)
    for sd, sg in zip(seeds, signs):
        p = oracle.prg(bytes(sd), len(w)).astype(np.uint64)
        acc = acc + p if sg > 0 else acc + (2 ** 32 - p)
    return (acc & 0xFFFFFFFF).astype(np.uint32), int(cl.sum())


# ------------------------------------------------------------------ case lists
def rotated_value_rows(frac_bits: int, clip: float, pack: int):
    """codec_cases.value_row(f, c) rotated by 0..P-1 places: every edge value in every field."""
    v = K.value_row(frac_bits, clip)
    return [np.roll(v, r) for r in range(pack)]


def worst_inputs(frac_bits: int, clip: float, n: int, L: int):
    """n clients' rows: every third at +c everywhere (the largest field, 2B, in every slot), the rest random with
    wild values; and their dither seeds, None (nearest) for every second client: mixed roundings."""
    xs, dithers = [], []
    for i in range(n):
        xs.append(np.full(L, clip, np.float32) if i % 3 == 0 else K.random_row(L, clip, 1000 + i, wild=True))
        dithers.append(None if i % 2 else bytes([i % 256, i // 256]) + bytes(30))
    return xs, dithers


def threshold_slots():
    """codec_cases.threshold_slots: [(parameter, r)] of DITHER's stream with 0 < r < 2^24."""
    return K.threshold_slots()


def threshold_row():
    """(x, [(parameter, r, thr, away)]) at (f = 7, c = 1): |t| = thr 2^-32 at the parameters of threshold_slots(),
    thr = r + 1 (rounds away from zero) and thr = r (truncates) in turn, both signs: x = +-thr 2^-32 2^-7 is an
    exact float32 for thr < 2^24.  The dither word of parameter l is PRG(DITHER)[l] whatever P is: a kernel
    that indexed the stream by word would round other parameters.  The other parameters hold fractions of all
    sizes inside +-c."""
    rng = np.random.default_rng(2077)
    x = (rng.random(K.THRESHOLD_L) * 1.5 - 0.75).astype(np.float32)
    picks = []
    for n, (l, r) in enumerate(threshold_slots()):
        away = n % 2 == 0
        thr = r + 1 if away else r
        sign = -1.0 if (n // 2) % 2 else 1.0
        x[l] = np.float32(sign * thr * 2.0 ** -32 * 2.0 ** -THRESHOLD_F)
        picks.append((l, r, thr, away))
    return x, picks
