"""Limb-exact model of mod_n_384 (flamingo_amd/csrc/flm_p256.hip): the reduction of a 384-bit value
mod the P-256 group order n that hash_to_curve_kernel applies to each half of expand_message_xmd's
96 bytes.

1. reduce(v) replays the kernel in Python integers: 12 limbs of 32 bits, ITERATIONS folds
   t = lo + hi (2^256 - n), each fold the 4 x 7 multiply-accumulate of hi's limbs by kNc with the
   kernel's carry order (the 64-bit accumulator c of row i runs over t[i .. i+6], then ripples
   through t[i+7 .. 11]), then one conditional subtraction of n (sc_below_n).  It asserts what the
   kernel assumes and cannot check: no accumulator value exceeds 64 bits, nothing carries out of
   limb 11, limbs 8..11 are zero after the loop, and one subtraction finishes.  It returns the
   residue and how many folds met a non-zero hi.
2. fold_bound() proves how many folds any 384-bit input can need.  With T the largest value before
   a fold and H = T >> 256, the largest value after it is
       max(T mod 2^256 + H Nc,  2^256 - 1 + (H - 1) Nc)
   (hi = H with the largest lo that T allows, or hi = H - 1 with lo = 2^256 - 1; Nc < 2^256, so no
   other (lo, hi) under T gives more), and both are reached.  From T = 2^384 - 1 the chain falls
   below 2^256 after five folds: 128 -> 96 -> 64 -> 32 -> 1 -> 0 bits of hi, since Nc < 2^224.
   The fifth is needed (about half of all inputs: after four folds hi is 0 or 1), a sixth never:
   the kernel's iterations 6 and 7 always see hi = 0 and add nothing.
3. FOLD_WITNESSES: one input for every count 0..5 (tests/test_h2c_cases_cpu.py checks them).
Run: python tools/h2c_reduce_model.py  (prints the bound chain and a fold-count histogram)"""
import random
from collections import Counter

N = 0xFFFFFFFF00000000FFFFFFFFFFFFFFFFBCE6FAADA7179E84F3B9CAC2FC632551
M32 = (1 << 32) - 1
# kNc of flm_p256.hip: 2^256 - n in 7 limbs, least significant first
NC_LIMBS = [0x039cdaaf, 0x0c46353d, 0x58e8617b, 0x43190552, 0x00000000, 0x00000000, 0xffffffff]
NC = sum(v << (32 * i) for i, v in enumerate(NC_LIMBS))
ITERATIONS = 7         # the kernel's loop count
MAX_FOLDS = 5          # fold_bound(): the most folds with a non-zero hi


def limbs(x, n=12):
    return [(x >> (32 * i)) & M32 for i in range(n)]


def val(w):
    return sum(v << (32 * i) for i, v in enumerate(w))


def fold(t):
    """One iteration of the kernel's loop on the 12 limbs t, in place; returns hi as an integer."""
    hi = t[8:12]
    before = val(t)
    t[8:12] = [0, 0, 0, 0]
    for i in range(4):
        c = 0
        for j in range(7):
            c = hi[i] * NC_LIMBS[j] + t[i + j] + (c >> 32)
            assert c < 1 << 64, "the accumulator overflows 64 bits"
            t[i + j] = c & M32
        c >>= 32
        for k in range(i + 7, 12):
            c += t[k]
            assert c < 1 << 64
            t[k] = c & M32
            c >>= 32
        assert c == 0, "carry out of limb 11"
    assert val(t) == (before & ((1 << 256) - 1)) + val(hi) * NC
    return val(hi)


def reduce(v, iterations=ITERATIONS):
    """(v mod n, folds with a non-zero hi) as mod_n_384 computes them; v < 2^384."""
    assert 0 <= v < 1 << 384
    t = limbs(v)
    folds = 0
    for _ in range(iterations):
        if fold(t):
            folds += 1
    assert t[8:12] == [0, 0, 0, 0], "limbs 8..11 are not zero after the loop"
    r = val(t[:8])
    assert r < 2 * N, "one subtraction of n does not finish the reduction"
    if r >= N:              # sc_below_n: mod_reduce_once<kN>(r, t, 0)
        r -= N
    assert r < N
    return r, folds


def fold_bound():
    """[T_0, T_1, ...]: the largest value before fold k over all 384-bit inputs, down to the first
    below 2^256.  len - 1 is the number of folds that can meet a non-zero hi."""
    R = 1 << 256
    chain = [(1 << 384) - 1]
    while chain[-1] >= R:
        T = chain[-1]
        H = T >> 256
        chain.append(max((T & (R - 1)) + H * NC, R - 1 + (H - 1) * NC))
        assert len(chain) <= ITERATIONS + 1, "the loop count is too small"
    return chain


# an input that needs exactly k folds, k = 0..MAX_FOLDS
FOLD_WITNESSES = {0: (1 << 256) - 1,
                  1: 1 << 256,
                  2: ((1 << 256) - NC) | (1 << 288),
                  3: ((1 << 256) - NC) | (1 << 320),
                  4: 1 << 383,
                  5: (1 << 384) - 1}


def histogram(n_random=20000, seed=384):
    rng = random.Random(seed)
    h = Counter()
    for _ in range(n_random):
        v = rng.getrandbits(384)
        r, f = reduce(v)
        assert r == v % N
        h[f] += 1
    return h


if __name__ == "__main__":
    chain = fold_bound()
    for k, T in enumerate(chain):
        print(f"largest value before fold {k + 1}: {T.bit_length()} bits, hi <= {T >> 256:#x}")
    print(f"at most {len(chain) - 1} folds meet a non-zero hi; the kernel runs {ITERATIONS}")
    for k, v in FOLD_WITNESSES.items():
        print(f"witness for {k} folds: {v:#x} -> {reduce(v)[1]}")
    print("fold counts of 20,000 random 384-bit inputs:", sorted(histogram().items()))
