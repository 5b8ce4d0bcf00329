"""The table-sampled (discrete Gaussian) noise share of the float codec (include/flamingo_hip.h)
restated in numpy on top of tests/dp_cases.py, and the case lists of its tests.  No test functions: the premises are
checked without a GPU by tests/test_dgauss_cpu.py, the kernels (encode_gauss_mask_kernel, and the packed decode at
noise_bits = 2 tau) bit for bit against them by tests/test_dgauss_gpu.py.

* draws_u64 / noise restate the sampler: the (high, low) words of parameter l are dp_cases.noise_words(seed, L, 64),
  u = high 2^32 + low, z = searchsorted(cdt, u, side="right") - tau: the number of entries <= u, less tau.
* bias_n / headroom_ok / length_ok / n_max restate the rules: B_n = B + tau in the binomial rule's B + b / 2.
* encode_any / decode_any / masked / batch_rows restate the codec with q' = q + z.
* TABLES, crafted tables, HEADROOM_EXAMPLES, gpu_cases: the case lists.
"""
from __future__ import annotations

import numpy as np

import codec_cases as K
import dp_cases as D
import pack_cases as PC
from codec_cases import oracle

REAL_TABLES = ((0.5, 5), (3.2, 32), (51.2, 512))       # (sigma, tau)
LENGTHS = D.LENGTHS
# dp_cases.HEADROOM_EXAMPLES and its unpacked edge with tau = b / 2: (f, c, P, tau, the largest n with headroom)
HEADROOM_EXAMPLES = tuple((f, c, P, b // 2, n) for f, c, P, b, n in D.HEADROOM_EXAMPLES + (D.UNPACKED_EDGE,))
ODD_TAU = 37                                            # T = 74: not a power of two


def real_table(sigma: float, tau: int) -> np.ndarray:
    from flamingo_amd import dgauss
    return dgauss.table(sigma, tau)


# ------------------------------------------------------------------ the sampler
def draws_u64(seed_: bytes, L: int) -> np.ndarray:
    """u(l) as uint64: ChaCha block 2 beta of PRG(seed) holds the high words of parameter block beta, 2 beta + 1 the low."""
    w = D.noise_words(seed_, L, 64).astype(np.uint64)
    return (w[:, 0] << np.uint64(32)) | w[:, 1]


def counts(seed_: bytes, L: int, cdt) -> np.ndarray:
    """#{j < T : cdt[j] <= u(l)} as int64, in [0, T]."""
    cdt = np.ascontiguousarray(cdt, np.uint64)
    assert cdt.ndim == 1 and len(cdt) % 2 == 0 and len(cdt) >= 2 and np.all(cdt[1:] >= cdt[:-1])
    return np.searchsorted(cdt, draws_u64(seed_, L), side="right").astype(np.int64)


def noise(seed_: bytes, L: int, cdt) -> np.ndarray:
    """z(l) = count - tau as int64, in [-tau, tau]."""
    return counts(seed_, L, cdt) - len(cdt) // 2


# ------------------------------------------------------------------ the rules
def bias_n(frac_bits: int, clip: float, tau: int) -> int:
    return PC.bias(frac_bits, clip) + tau


def headroom_ok(frac_bits: int, clip: float, pack: int, tau: int, n: int) -> bool:
    return D.headroom_ok(frac_bits, clip, pack, 2 * tau, n)          # B + b / 2 at b = 2 tau


def n_max(frac_bits: int, clip: float, pack: int, tau: int) -> int:
    return D.n_max(frac_bits, clip, pack, 2 * tau)


def length_ok(L: int) -> bool:
    return 2 * -(-L // 16) <= 2 ** 32


# ------------------------------------------------------------------ the codec with the noise
def quantised(x, frac_bits, clip, cdt, noise_seed, dither=None):
    """(q' = q + z per parameter as int64, clipped mask): the clipped mask is that of the call without noise."""
    w, clipped = K.encode(x, frac_bits, clip, dither)
    q = w.view(np.int32).astype(np.int64)
    return q + noise(noise_seed, len(q), cdt), clipped


def encode_any(x, frac_bits, clip, pack, cdt, noise_seed, dither=None):
    """(ring words, clipped mask).  Unpacked uint32(q'); packed the field q' + B_n = q + B + count in [0, 2 B_n]."""
    q, clipped = quantised(x, frac_bits, clip, cdt, noise_seed, dither)
    if pack == 1:
        return (q & 0xFFFFFFFF).astype(np.uint32), clipped
    bn = bias_n(frac_bits, clip, len(cdt) // 2)
    u = q + bn
    assert np.all((u >= 0) & (u <= 2 * bn))
    return PC.pack_fields(u, pack), clipped


def decode_any(S, L, frac_bits, clip, pack, tau, count=1):
    """The binomial restatement's decode at noise_bits = 2 tau: B_n = B + tau."""
    return D.decode_any(S, L, frac_bits, clip, pack, 2 * tau, count)


def masked(x, frac_bits, clip, pack, seeds, signs, cdt, noise_seed, dither=None):
    """encode(x) with noise + sum_k signs[k] PRG(seeds[k]) mod 2^32 over the words -> (row, clipped elements)."""
    w, cl = encode_any(x, frac_bits, clip, pack, cdt, noise_seed, dither)
    acc = w.astype(np.uint64)
    for sd, sg in zip(seeds, signs):
        p = oracle.prg(bytes(sd), len(w)).astype(np.uint64)
        acc = acc + p if sg > 0 else acc + (2 ** 32 - p)
    return (acc & 0xFFFFFFFF).astype(np.uint32), int(cl.sum())


def batch_rows(xs, seg, seeds, signs, frac_bits, clip, pack, dithers, noises, cdt):
    """The restatement of one batch call: (rows, clipped counts)."""
    rows, cl = [], []
    for i in range(len(xs)):
        r, c = masked(xs[i], frac_bits, clip, pack, seeds[seg[i]:seg[i + 1]], signs[seg[i]:seg[i + 1]], cdt, noises[i],
                      dithers[i] if dithers is not None else None)
        rows.append(r)
        cl.append(c)
    return np.stack(rows), np.array(cl, np.uint32)


# ------------------------------------------------------------------ crafted tables
def all_zeros(tau: int) -> np.ndarray:
    """Every entry <= every draw: every z = +tau."""
    return np.zeros(2 * tau, np.uint64)


def all_ones(tau: int) -> np.ndarray:
    """Every entry 2^64 - 1: every z = -tau (unless a draw is 2^64 - 1 itself)."""
    return np.full(2 * tau, 2 ** 64 - 1, np.uint64)


def coin() -> np.ndarray:
    """tau = 1, [2^63, 2^63]: z = -1 below 2^63 and +1 from it on, never 0: the off-by-one of the rule."""
    return np.array([2 ** 63, 2 ** 63], np.uint64)


def even_steps(tau: int = ODD_TAU) -> np.ndarray:
    """Strictly increasing entries spaced 2^64 / (T + 1): every count 0..T has the same chance."""
    T = 2 * tau
    return np.array([(j + 1) * 2 ** 64 // (T + 1) for j in range(T)], np.uint64)


def low_word_table(hi: int, tau: int = 4) -> np.ndarray:
    """Entries that share the high word `hi` and differ only in the low word, evenly spread over it."""
    T = 2 * tau
    return np.array([(hi << 32) | ((j + 1) * 2 ** 32 // (T + 1)) for j in range(T)], np.uint64)


def top_bit_table(tau: int = 4) -> np.ndarray:
    """Entries from 2^63 up, evenly spread: entries and draws on both sides of bit 63, where a signed compare of the
    high half inverts the order."""
    T = 2 * tau
    return np.array([2 ** 63 + j * 2 ** 63 // T for j in range(T)], np.uint64)


# ------------------------------------------------------------------ case lists
def gpu_params(tau: int):
    """(P, f, c): every width with the (f, c) of pack_cases.VALUE_PARAMS at which one client has headroom at tau
    (P = 4 admits (2, 1) alone, and tau <= 123 there)."""
    return [(P, f, c) for P in (1, 2, 4) for f, c in PC.VALUE_PARAMS if headroom_ok(f, c, P, tau, 1)]
