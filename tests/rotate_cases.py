"""The randomised block Hadamard rotation of float updates (include/flamingo_hip.h) restated in
numpy on top of oracle.prg, and the case lists of its tests.  No test functions: the premises are checked without a GPU
by tests/test_rotate_cpu.py, the kernel (rotate_kernel) bit for bit against them by tests/test_rotate_gpu.py.

* sign_words / sign_mask / c_h / rotated_len / forward / inverse restate the transform, stage by stage over a reshaped
  array: every add has fixed operands, so the float32 result is one bit pattern whatever order evaluates the stages'
  pairs.  Nothing here is a matrix product.
* hadamard64: the same block transform as a float64 matrix product, the yardstick of the accuracy bound.
* lengths(h): the row lengths of the GPU cases; ONE_HOT: the one-hot claim of the issue this feature answers.
"""
from __future__ import annotations

import hashlib

import numpy as np

import codec_cases as K
from codec_cases import oracle

LOG2_BLOCKS = tuple(range(4, 13))
KEY = hashlib.sha256(b"rotation key").digest()
KEY2 = hashlib.sha256(b"another rotation key").digest()
RSQRT2_BITS = 0x3F3504F3                       # float32(sqrt(1 / 2))
# n clients hold one-hots of height 1.0 at these positions: L, h, frac_bits, clip, pack
ONE_HOT = dict(positions=(0, 63, 64, 99, 5, 5, 70, 31), L=100, h=6, f=7, c=0.25, pack=2)


def lengths(h: int):
    H = 1 << h
    return (1, H - 1, H, H + 1, 4095, 4096, 4097, 2 * 4096 + H // 2 + 3)


# ------------------------------------------------------------------ the transform
def rotated_len(L: int, h: int) -> int:
    H = 1 << h
    return -(-L // H) * H


def sign_words(key: bytes, L_rot: int) -> np.ndarray:
    """ceil(L_rot / 32) words of PRG(key): what the device form is given."""
    return oracle.prg(key, -(-L_rot // 32))


def sign_mask(key: bytes, L_rot: int) -> np.ndarray:
    """uint32 per parameter: 0x80000000 where parameter l is negated, bit l % 32 of word l // 32."""
    w = sign_words(key, L_rot)
    l = np.arange(L_rot)
    return (((w[l // 32] >> (l % 32).astype(np.uint32)) & np.uint32(1)) << np.uint32(31)).astype(np.uint32)


def c_h(h: int) -> np.float32:
    """float32(2^(-h / 2)): a power of two, times 0x3F3504F3 for odd h."""
    m = np.array([RSQRT2_BITS], np.uint32).view(np.float32)[0] if h % 2 else np.float32(1.0)
    return np.float32(m * np.float32(2.0 ** -(h // 2)))    # exact: a power-of-two multiple


def _flip(v: np.ndarray, mask: np.ndarray) -> np.ndarray:
    return (np.ascontiguousarray(v, np.float32).view(np.uint32) ^ mask).view(np.float32)


def _stages(v: np.ndarray, h: int) -> np.ndarray:
    """Stages 0 .. h - 1 in that order on blocks of 2^h of the flat float32 array v, then the multiply by c_h."""
    v = np.ascontiguousarray(v, np.float32).copy()
    with np.errstate(over="ignore", invalid="ignore"):
        for s in range(h):
            p = v.reshape(-1, 2, 1 << s)                     # [..., bit s of the index, the bits below it]
            a, b = p[:, 0, :].copy(), p[:, 1, :].copy()
            p[:, 0, :] = a + b                               # float32 adds, round to nearest
            p[:, 1, :] = a - b
        return (v * c_h(h)).astype(np.float32)


def forward(x, key: bytes, h: int):
    """(the L_rot rotated floats, the number of non-finite inputs) of one row x of L floats."""
    x = np.asarray(x, np.float32)
    assert x.ndim == 1 and 4 <= h <= 12 and len(x) > 0
    L_rot = rotated_len(len(x), h)
    v = np.zeros(L_rot, np.float32)                          # parameters >= L read as +0.0
    bad = ~np.isfinite(x)
    v[:len(x)] = np.where(bad, np.float32(0.0), x)
    return _stages(_flip(v, sign_mask(key, L_rot)), h), int(bad.sum())


def inverse(y, key: bytes, h: int, L: int) -> np.ndarray:
    """The first L parameters of the row whose rotation is y (L_rot floats): stages, multiply, sign flips."""
    y = np.asarray(y, np.float32)
    assert y.ndim == 1 and len(y) == rotated_len(L, h)
    return _flip(_stages(y, h), sign_mask(key, len(y)))[:L].copy()


def hadamard64(v, h: int) -> np.ndarray:
    """2^(-h / 2) H_{2^h} applied to every block of the flat array v, in float64, as a matrix product."""
    H = np.array([[1.0]])
    for _ in range(h):
        H = np.block([[H, H], [H, -H]])
    return (np.asarray(v, np.float64).reshape(-1, 1 << h) @ H.T).reshape(-1) * 2.0 ** (-h / 2.0)


def error_bound(x_block_norm: float, h: int) -> float:
    """|fl(y) - y| <= (h + 1) 2^-24 ||x_block||_2 per element of a block."""
    return (h + 1) * 2.0 ** -24 * x_block_norm


# ------------------------------------------------------------------ case lists
def rows(N: int, L: int, seed: int) -> np.ndarray:
    """N rows of L finite floats of mixed magnitude."""
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((N, L)) * np.exp(rng.uniform(-6, 3, (N, L)))).astype(np.float32)


def bits(a) -> np.ndarray:
    """The comparison of the GPU tests: NaN compares as NaN (one canonical pattern), everything else by its bits."""
    a = np.ascontiguousarray(a, np.float32)
    return np.where(np.isnan(a), np.uint32(0x7FC00000), a.view(np.uint32))


def one_hot_clients():
    c = ONE_HOT
    xs = np.zeros((len(c["positions"]), c["L"]), np.float32)
    xs[np.arange(len(c["positions"])), list(c["positions"])] = 1.0
    return xs


def codec_mean(xs, frac_bits: int, clip: float, pack: int):
    """The packed nearest-even codec around the plain sum of the rows: (mean float32, clipped per row, max |q|)."""
    import pack_cases as PC
    total, clipped, qmax = 0, [], 0
    for x in xs:
        w, cl = PC.encode_packed(x, frac_bits, clip, pack)
        q = K.encode(x, frac_bits, clip)[0].view(np.int32)
        total = (total + w.astype(np.uint64)) & 0xFFFFFFFF
        clipped.append(int(cl.sum()))
        qmax = max(qmax, int(np.abs(q).max()))
    return PC.decode_packed(total.astype(np.uint32), xs.shape[1], frac_bits, clip, pack, len(xs)), clipped, qmax
