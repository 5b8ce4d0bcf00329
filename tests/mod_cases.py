"""The decode modulo the field (include/flamingo_hip.h "decode modulo the field") restated in numpy
on top of tests/pack_cases.py and tests/dp_cases.py, with a big-integer model beside it, and the case lists of its tests.
No test functions: the restatement is held against the model without a GPU by tests/test_mod_cpu.py, the kernels
(decode_unpack_mod_kernel) bit for bit against the restatement by tests/test_mod_gpu.py.

* half / modulus / admitted restate the widths and the admission: 2 B_n <= M - 1 and 1 <= n <= 2^31 - 1.
* summed_words(Q, pack, n, B_n): the word a ring sum leaves when the signed field sums are Q: sum_j (Q_j + n B_n) <<
  (W j) mod 2^32, carries between the fields allowed.  No encoding is needed to build a case.
* decode_mod: the rule's cascade in uint32 numpy -> (float32 means, Qh as int64).
* model_word(Q_word, pack): property 3 in Python integers, from the field sums alone: Qh_j = centred((Q_j + k_{j-1})
  mod M), k_j = (Q_j + k_{j-1} - Qh_j) / M.
* rule_word(S, pack, n, B_n): the rule itself in Python integers, from the word.
* stats(Qh, guard): (#{|Qh| >= guard}, max |Qh|).
* edge_q / handoff_words / edge_row / random_q: the field sums of the cases.
* ROUNDS / round_case: the end-to-end rounds the worst-case rule refuses, encoded on the CPU.
"""
from __future__ import annotations

import math
from fractions import Fraction

import numpy as np

import codec_cases as K
import dgauss_cases as G
import dp_cases as D
import pack_cases as PC
from flamingo_amd import modular          # the caller's side of the feature; half and guard below restate it

PACKS = PC.PACKS
MAX_COUNT = 2 ** 31 - 1
assert all(modular.half_modulus(P) == 2 ** (32 // P - 1) for P in PACKS)


def shapes(pack: int):
    """Below a quad, a quad less one, a quad, a quad and one, more than one block, an odd length."""
    P = pack
    return (1, 4 * P - 1, 4 * P, 4 * P + 1, 1025, 2077)


def long_shape(pack: int) -> int:
    """4096 groups of 256 threads take 2^20 quads a trip: a second trip of one quad, and a tail of 3 parameters."""
    return 4 * pack * 2 ** 20 + 4 * pack + 3


# (f, c, noise_bits, n) that both widths admit.  B_n = 3: n B_n = 15 below either M; 90000 at or above either M (a carry
# into the next field); the issue's example 3 (2^31 - 1) at or above 2^32.  B_n = ceil(1.9 * 64) + 5 = 127, the largest
# P = 4 admits, with the largest count.
BIAS_CASES = ((0, 1.0, 4, 5), (0, 1.0, 4, 30000), (0, 1.0, 4, MAX_COUNT), (6, 1.9, 10, MAX_COUNT))


# ------------------------------------------------------------------ the rule
def modulus(pack: int) -> int:
    return 2 ** (32 // pack)


def half(pack: int) -> int:
    return 2 ** (32 // pack - 1)


def guard(pack: int, fraction: float) -> int:
    """flamingo_amd.modular.guard restated: ceil(fraction H) clamped to 1..H."""
    return min(half(pack), max(1, math.ceil(Fraction(float(fraction)) * half(pack))))


def admitted(frac_bits: int, clip: float, pack: int, noise_bits: int, n: int) -> bool:
    return 2 * D.bias_n(frac_bits, clip, noise_bits) <= modulus(pack) - 1 and 1 <= n <= MAX_COUNT


def summed_words(Q, pack: int, n: int, bn: int) -> np.ndarray:
    """ceil(L / P) words uint32 from L signed field sums; fields past L hold 0 (no contributor put a bias there)."""
    Q = np.asarray(Q, np.int64)
    W, Lw = 32 // pack, -(-len(Q) // pack)
    T = np.zeros(Lw * pack, np.int64)
    assert np.all(np.abs(Q) < 2 ** 40) and 0 <= n * bn < 2 ** 47      # n < 2^31, B_n < 2^15: the sum stays in int64
    T[:len(Q)] = (Q + n * bn) & 0xFFFFFFFF        # T mod 2^32, which is all the word keeps: shifted terms below 2^56
    terms = T.reshape(Lw, pack) << (W * np.arange(pack, dtype=np.int64))
    return (terms.sum(axis=1) & 0xFFFFFFFF).astype(np.uint32)


def decode_mod(S, L: int, frac_bits: int, pack: int, n: int, bn: int):
    """The cascade in uint32: (out float32[L], Qh int64[L])."""
    S = np.ascontiguousarray(S, np.uint32)
    assert len(S) == -(-L // pack)
    W, M, H = 32 // pack, modulus(pack), half(pack)
    cb = np.uint32((n * bn) % 2 ** 32)
    r = S.copy()
    qh = np.empty((len(S), pack), np.int64)
    with np.errstate(over="ignore"):
        for j in range(pack):
            d = (r - cb).astype(np.uint32)
            v = (d & np.uint32(M - 1)).astype(np.int64)
            q = v - M * (v >= H)
            r = ((d - (q & 0xFFFFFFFF).astype(np.uint32)).astype(np.uint32) >> np.uint32(W)).astype(np.uint32)
            qh[:, j] = q
    qh = qh.reshape(-1)[:L]
    out = (qh.astype(np.float64) / (np.float64(n) * 2.0 ** frac_bits)).astype(np.float32)
    return out, qh


def stats(qh, guard_: int):
    a = np.abs(np.asarray(qh, np.int64))
    return int((a >= guard_).sum()), int(a.max()) if len(a) else 0


# ------------------------------------------------------------------ the models, in Python integers
def centred(t: int, pack: int) -> int:
    M, H = modulus(pack), half(pack)
    return (t + H) % M - H


def model_word(q_word, pack: int):
    """([Qh_j], [k_j]) from the field sums of one word: property 3."""
    M = modulus(pack)
    k, qh, ks = 0, [], []
    for q in q_word:
        t = int(q) + k
        c = centred(t, pack)
        assert (t - c) % M == 0
        k = (t - c) // M
        qh.append(c)
        ks.append(k)
    return qh, ks


def rule_word(S: int, pack: int, n: int, bn: int):
    """[Qh_j] from the summed word: the rule line by line."""
    W, M, H = 32 // pack, modulus(pack), half(pack)
    cb, r, out = (n * bn) % 2 ** 32, int(S), []
    for _ in range(pack):
        d = (r - cb) % 2 ** 32
        v = d % M
        q = v - M * (v >= H)
        assert (d - q) % 2 ** 32 % M == 0
        r = ((d - q) % 2 ** 32) >> W
        out.append(q)
    return out


def word_of(q_word, pack: int, n: int, bn: int) -> int:
    W = 32 // pack
    return sum((int(q) + n * bn) << (W * j) for j, q in enumerate(q_word)) % 2 ** 32


# ------------------------------------------------------------------ case lists
def edge_q(pack: int, guard_: int):
    """In-range field sums at the ends of the range, around zero and around the guard (a guard of H itself is reached
    by -H alone: +H is not in range)."""
    H = half(pack)
    return [v for v in (-H, H - 1, -1, 0, guard_ - 1, guard_, -guard_) if -H <= v < H]


def handoff_words(pack: int):
    """[(Q of one word, the k its low field hands up)]: the low field wrapped by k M, k = +-1 and +-2, the fields above
    it in range, so that Qh of field 1 is Q_1 + k; and one where the hand-off wraps the field above in turn."""
    M, H = modulus(pack), half(pack)
    out = []
    for k in (1, -1, 2, -2):
        for low in (k * M, k * M + 5, k * M - H, k * M + H - 1):
            out.append(([low] + [7 * (j + 1) for j in range(pack - 1)], k))
    out.append(([M + 3, H - 1] + [0] * (pack - 2), 1))        # H - 1 + 1 = H wraps to -H and hands 1 further up
    return out


def edge_row(pack: int, guard_: int, L: int) -> np.ndarray:
    """L in-range field sums: edge_q's values in turn, shifted by one place per word so that every value meets every
    field, the rest random inside [-H, H - 1]."""
    H = half(pack)
    rng = np.random.default_rng(4000 + 10 * L + pack)
    q = rng.integers(-H, H, size=L, dtype=np.int64)
    e = edge_q(pack, guard_)
    for i in range(min(L, 4 * len(e) * pack)):
        q[i] = e[(i + i // pack) % len(e)]
    return q


def random_q(pack: int, L: int, seed_: int, wrapped: bool = False) -> np.ndarray:
    """Random field sums: inside [-H, H - 1], or (wrapped) up to 3 M beyond it on either side."""
    H, M = half(pack), modulus(pack)
    rng = np.random.default_rng(seed_)
    return rng.integers(-H - 3 * M, H + 3 * M, size=L, dtype=np.int64) if wrapped else rng.integers(-H, H, size=L, dtype=np.int64)


# (f, c, P, rounding, n, L, noise): the issue's rounds.  noise: None, ("table", sigma, tail) or ("binomial", b)
ROUNDS = ((7, 1.0, 2, "stochastic", 600, 2077, None),
          (2, 1.0, 4, "nearest", 100, 2077, None),
          (4, 1.0, 2, "stochastic", 1500, 1025, ("table", 3.2, 32)),
          (4, 1.0, 2, "nearest", 2200, 1025, ("binomial", 30)))


def round_noise_bits(noise) -> int:
    return 0 if noise is None else 2 * noise[2] if noise[0] == "table" else noise[1]


def round_inputs(c: float, rounding: str, n: int, L: int, noise):
    """(x (n, L) float32, dither seeds or None, noise seeds or None): rows codec_cases.random_row(L, c, 1000 + i), noise
    seeds dp_cases.seed(i), dither seeds dp_cases.seed(10000 + i)."""
    xs = np.stack([K.random_row(L, c, 1000 + i) for i in range(n)])
    dithers = [D.seed(10000 + i) for i in range(n)] if rounding == "stochastic" else None
    noises = [D.seed(i) for i in range(n)] if noise is not None else None
    return xs, dithers, noises


def round_case(f: int, c: float, pack: int, rounding: str, n: int, L: int, noise):
    """The round on the CPU: (Q int64[L], the signed sums of the clients' q'; S uint32, the sum of their packed words mod
    2^32).  Every client's word is the parent's encode, restated by pack_cases, dp_cases and dgauss_cases."""
    xs, dithers, noises = round_inputs(c, rounding, n, L, noise)
    cdt = G.real_table(noise[1], noise[2]) if noise is not None and noise[0] == "table" else None
    Q = np.zeros(L, np.int64)
    S = np.zeros(-(-L // pack), np.uint64)
    for i in range(n):
        dz = dithers[i] if dithers is not None else None
        if noise is None:
            w, _ = K.encode(xs[i], f, c, dz)
            q = w.view(np.int32).astype(np.int64)
            words = PC.pack_fields(q + PC.bias(f, c), pack)
        elif noise[0] == "table":
            q, _ = G.quantised(xs[i], f, c, cdt, noises[i], dz)
            words = G.encode_any(xs[i], f, c, pack, cdt, noises[i], dz)[0]
        else:
            q, _ = D.quantised(xs[i], f, c, dz, noises[i], noise[1])
            words = D.encode_packed_noised(xs[i], f, c, pack, dz, noises[i], noise[1])[0]
        Q += q
        S += words
    return Q, (S & 0xFFFFFFFF).astype(np.uint32)
