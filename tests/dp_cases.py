"""The distributed-DP binomial noise of the float codec (include/flamingo_hip.h) restated in
numpy on top of tests/codec_cases.py and tests/pack_cases.py, and the case lists of its tests.  No test functions:
the premises are checked without a GPU by tests/test_dp_cpu.py, the kernels (encode_mask_kernel with noise and the
packed decode with the noised bias) bit for bit against them by tests/test_dp_gpu.py.

* draws / noise_words / noise restate the mechanism: b = noise_bits fair coins per parameter and client,
  m = ceil(b / 32) draws, draw d of parameter l is PRG(seed)[16 (m (l // 16) + d) + l % 16], the last draw ANDed
  with 2^r - 1 when r = b mod 32 is not 0, Z[l] = sum_d popcount(draw) - b / 2.
* bias_n / headroom_ok / length_ok / n_max restate the rules: B_n = B + b / 2, unpacked n B_n <= 2^31 - 1, packed
  n 2 B_n <= 2^W - 1, m ceil(L / 16) <= 2^32.
* encode_noised / encode_packed_noised / decode_packed_noised / masked_noised restate the codec with q' = q + Z.
* HEADROOM_EXAMPLES, UNPACKED_EDGE, GPU_CASES, GPU_ROUNDS: the case lists.
"""
from __future__ import annotations

import hashlib

import numpy as np

import codec_cases as K
import pack_cases as PC
from codec_cases import oracle

NOISE_BITS = (2, 30, 32, 34, 160, 1024)      # r = 0 and r != 0, m = 1, more noise units than waves, the maximum
LENGTHS = (17, 1025, 2077)
BATCH_SEEDS = (0, 1, 5, 14)                  # seeds of the four clients of a batch
# (f, c, P, b, the largest n with headroom); the third: at n = 255 no b > 0 has room
HEADROOM_EXAMPLES = ((4, 1.0, 2, 30, 1057), (2, 1.0, 4, 2, 25))
NO_ROOM = (7, 1.0, 2, 255)
# unpacked: B = 4 2^16 = 262144, b = 1024, B_n = 262656; 8176 B_n = 2147475456 <= 2^31 - 1 < 8177 B_n = 2147738112
UNPACKED_EDGE = (16, 4.0, 1, 1024, 8176)
GPU_ROUNDS = ((2, 1.0, 4, 2, 25, 2077), (16, 4.0, 1, 64, 64, 2077))   # (f, c, P, b, n, L)


def seed(i: int) -> bytes:
    return hashlib.sha256(b"dp noise %d" % i).digest()


# ------------------------------------------------------------------ the noise
def draws(b: int) -> int:
    return -(-b // 32)


def noise_words(seed_: bytes, L: int, b: int) -> np.ndarray:
    """w(l, d) as an (L, m) uint32 array, the last draw already masked."""
    m, r, blocks = draws(b), b % 32, -(-L // 16)
    stream = oracle.prg(seed_, 16 * m * blocks).reshape(blocks, m, 16)    # block m beta + d: draw d of block beta
    w = stream.transpose(0, 2, 1).reshape(blocks * 16, m)[:L].copy()
    if r:
        w[:, m - 1] &= np.uint32(2 ** r - 1)
    return w


def popcount(w: np.ndarray) -> np.ndarray:
    return np.unpackbits(np.ascontiguousarray(w, np.uint32).view(np.uint8).reshape(w.shape + (4,)), axis=-1).sum(axis=-1).astype(np.int64)


def noise(seed_: bytes, L: int, b: int) -> np.ndarray:
    """Z[l] = sum_d popcount(w(l, d)) - b / 2 as int64; zeros when b = 0."""
    if b == 0:
        return np.zeros(L, np.int64)
    assert b % 2 == 0 and 2 <= b <= 1024
    return popcount(noise_words(seed_, L, b)).sum(axis=1) - b // 2


# ------------------------------------------------------------------ the rules
def bias_n(frac_bits: int, clip: float, b: int) -> int:
    return PC.bias(frac_bits, clip) + b // 2


def headroom_ok(frac_bits: int, clip: float, pack: int, b: int, n: int) -> bool:
    """The worst case in exact integers: unpacked n B_n <= 2^31 - 1, packed n 2 B_n <= 2^W - 1."""
    if pack == 1:
        return n * bias_n(frac_bits, clip, b) <= 2 ** 31 - 1
    return n * 2 * bias_n(frac_bits, clip, b) <= 2 ** (32 // pack) - 1


def length_ok(b: int, L: int) -> bool:
    return draws(b) * -(-L // 16) <= 2 ** 32


def n_max(frac_bits: int, clip: float, pack: int, b: int) -> int:
    top = 2 ** 31 - 1 if pack == 1 else 2 ** (32 // pack) - 1
    return top // (bias_n(frac_bits, clip, b) * (1 if pack == 1 else 2))


# ------------------------------------------------------------------ the codec with noise
def quantised(x, frac_bits, clip, dither=None, noise_seed=None, b=0):
    """(q' = q + Z per parameter as int64, clipped mask): the clipped mask is that of the call without noise."""
    w, clipped = K.encode(x, frac_bits, clip, dither)
    q = w.view(np.int32).astype(np.int64)
    return q + (noise(noise_seed, len(q), b) if b else 0), clipped


def encode_noised(x, frac_bits, clip, dither=None, noise_seed=None, b=0):
    """Unpacked: (ring words uint32(q'), clipped mask)."""
    q, clipped = quantised(x, frac_bits, clip, dither, noise_seed, b)
    return (q & 0xFFFFFFFF).astype(np.uint32), clipped


def encode_packed_noised(x, frac_bits, clip, pack, dither=None, noise_seed=None, b=0):
    """Packed: field u = q' + B_n in [0, 2 B_n]; (ceil(L / P) ring words, clipped mask)."""
    q, clipped = quantised(x, frac_bits, clip, dither, noise_seed, b)
    u = q + bias_n(frac_bits, clip, b)
    assert np.all((u >= 0) & (u <= 2 * bias_n(frac_bits, clip, b)))
    return PC.pack_fields(u, pack), clipped


def decode_packed_noised(S, L, frac_bits, clip, pack, b, count=1):
    """pack_cases.decode_packed with B_n in B's place."""
    S = np.ascontiguousarray(S, np.uint32).astype(np.int64)
    W = 32 // pack
    assert len(S) == -(-L // pack)
    s = (S[:, None] >> (W * np.arange(pack, dtype=np.int64))) & (2 ** W - 1)
    v = (s.reshape(-1)[:L] - count * bias_n(frac_bits, clip, b)).astype(np.float64)
    return (v / (np.float64(count) * 2.0 ** frac_bits)).astype(np.float32)


def encode_any(x, frac_bits, clip, pack, dither=None, noise_seed=None, b=0):
    if pack == 1:
        return encode_noised(x, frac_bits, clip, dither, noise_seed, b)
    return encode_packed_noised(x, frac_bits, clip, pack, dither, noise_seed, b)


def decode_any(S, L, frac_bits, clip, pack, b, count=1):
    if pack == 1:
        return K.decode(S, frac_bits, count)
    return decode_packed_noised(S, L, frac_bits, clip, pack, b, count)


def masked_noised(x, frac_bits, clip, pack, seeds, signs, dither=None, noise_seed=None, b=0):
    """encode(x) with noise + sum_k signs[k] PRG(seeds[k]) mod 2^32 over the words -> (row, clipped elements)."""
    w, cl = encode_any(x, frac_bits, clip, pack, dither, noise_seed, b)
    acc = w.astype(np.uint64)
    for sd, sg in zip(seeds, signs):
        p = oracle.prg(bytes(sd), len(w)).astype(np.uint64)
        acc = acc + p if sg > 0 else acc + (2 ** 32 - p)
    return (acc & 0xFFFFFFFF).astype(np.uint32), int(cl.sum())


def expected_std(frac_bits: int, b: int, count: int) -> float:
    """Standard deviation of the noise in the decoded mean over `count` contributors."""
    return float(np.sqrt(count * b) / (2.0 * count * 2.0 ** frac_bits))


# ------------------------------------------------------------------ case lists
def gpu_cases():
    """(P, f, c, b): every width, the (f, c) of pack_cases.VALUE_PARAMS and every b of NOISE_BITS at which one
    client has headroom (P = 4 admits (2, 1) alone, and b <= 246 there)."""
    return [(P, f, c, b) for P in (1, 2, 4) for f, c in PC.VALUE_PARAMS for b in NOISE_BITS if headroom_ok(f, c, P, b, 1)]


def batch(L: int, clip: float, tag: int):
    """Four clients with 0, 1, 5 and 14 seeds: (xs, seg, seeds, signs, dither seeds, noise seeds).  The rows hold wild
    values (NaN, infinities, beyond the clip) so that the clipped counts are not zero."""
    rng = np.random.default_rng(1000 * tag + L)
    K_ = sum(BATCH_SEEDS)
    seeds = rng.integers(0, 256, size=(K_, 32), dtype=np.uint8)
    signs = rng.choice(np.array([-1, 1], np.int8), size=K_)
    seg = np.concatenate([[0], np.cumsum(BATCH_SEEDS)]).astype(np.int64)
    xs = np.stack([K.random_row(L, clip, 50 * tag + i, wild=True) for i in range(len(BATCH_SEEDS))])
    dithers = [hashlib.sha256(b"dp dither %d %d" % (tag, i)).digest() for i in range(len(BATCH_SEEDS))]
    noises = [seed(100 * tag + i) for i in range(len(BATCH_SEEDS))]
    return xs, seg, seeds, signs, dithers, noises


def batch_rows(xs, seg, seeds, signs, frac_bits, clip, pack, dithers, noises, b):
    """The restatement of one batch call: (rows, clipped counts)."""
    rows, cl = [], []
    for i in range(len(xs)):
        r, c = masked_noised(xs[i], frac_bits, clip, pack, seeds[seg[i]:seg[i + 1]], signs[seg[i]:seg[i + 1]],
                             dithers[i] if dithers is not None else None, noises[i] if b else None, b)
        rows.append(r)
        cl.append(c)
    return np.stack(rows), np.array(cl, np.uint32)
