"""Model of the GPU inversion: Pornin's optimized binary GCD (eprint 2020/972, Alg. 2) with
k-1 = 30 inner steps (int32 update factors), 64-bit approximations (low 30 bits + top 34 bits).

inv(..., trace={}) also records what the schedule did on that input (outer steps count from 1):
  done      the outer step after which a == 0 (None: never)
  settled   the outer step after which b == 1: from then on only a and u change, so the result v is
            final (the kernel returns v and never looks at a); settled <= done
  nga, ngb  the outer steps at which a (b) came out negative and was negated with its matrix row
  windows   per outer step (q, aligned): q = sh >> 5 the limb the kernel's window starts in,
            aligned = (sh & 31 == 0)
  short     the outer steps run with both operands shorter than 64 bits (sh clamped to 0)
  pow30     the outer steps at which an update factor reached +-2^30 (empty: never; once a == 0
            every step does, with g1 = 2^30)
  quot      per outer step, the range each of the two bg_lin_modp quotients (new u, new v) fell in
            before the final correction: QUOT_RANGES = [-m, 0), [0, m), [m, 2^256), [2^256, 2m]"""
import random
P = 2**256 - 2**224 + 2**192 + 2**96 - 1
M64 = (1 << 64) - 1
QUOT_RANGES = ("neg", "plain", "above_m", "above_2_256")


def _quot_range(w, mod):
    return QUOT_RANGES[0 if w < 0 else 1 if w < mod else 2 if w < (1 << 256) else 3]


def inv(x, outer=18, trace=None, mod=P):
    """x^-1 mod `mod` (odd, below 2^256): p by default, the group order n for the ECDSA kernel"""
    a, b, u, v = x, mod, 1, 0
    ninv30 = (-pow(mod, -1, 1 << 30)) % (1 << 30)           # 1 for p
    if trace is not None:
        trace.update(nga=[], ngb=[], windows=[], short=[], pow30=[], quot=[])
    for it in range(outer):
        n = max(a.bit_length(), b.bit_length(), 64)
        sh = n - 64
        if trace is not None:
            trace['windows'].append((sh >> 5, sh & 31 == 0))
            if max(a.bit_length(), b.bit_length()) < 64: trace['short'].append(it + 1)
        abar = ((a >> sh) & ~((1 << 30) - 1) & M64) | (a & ((1 << 30) - 1))
        bbar = ((b >> sh) & ~((1 << 30) - 1) & M64) | (b & ((1 << 30) - 1))
        f0, g0, f1, g1 = 1, 0, 0, 1
        for j in range(30):
            if abar & 1:
                if abar < bbar:
                    abar, bbar = bbar, abar
                    f0, g0, f1, g1 = f1, g1, f0, g0
                abar -= bbar
                f0, g0 = f0 - f1, g0 - g1
            abar >>= 1
            f1, g1 = 2 * f1, 2 * g1
        assert max(abs(f0), abs(g0), abs(f1), abs(g1)) <= 2**30
        na, nb = a * f0 + b * g0, a * f1 + b * g1
        assert na % (1 << 30) == 0 and nb % (1 << 30) == 0
        na >>= 30; nb >>= 30
        if trace is not None:
            if max(abs(f0), abs(g0), abs(f1), abs(g1)) == 2**30: trace['pow30'].append(it + 1)
            if na < 0: trace['nga'].append(it + 1)
            if nb < 0: trace['ngb'].append(it + 1)
        if na < 0: na, f0, g0 = -na, -f0, -g0
        if nb < 0: nb, f1, g1 = -nb, -f1, -g1
        a, b = na, nb
        w0, w1 = u * f0 + v * g0, u * f1 + v * g1
        q0, q1 = w0 * ninv30 % (1 << 30), w1 * ninv30 % (1 << 30)      # -p^-1 = 1 mod 2^30
        assert (w0 + q0 * mod) % (1 << 30) == 0 and (w1 + q1 * mod) % (1 << 30) == 0
        u, v = (w0 + q0 * mod) >> 30, (w1 + q1 * mod) >> 30
        assert -mod <= u <= 2 * mod and -mod <= v <= 2 * mod, (u, v)
        if trace is not None: trace['quot'].append((_quot_range(u, mod), _quot_range(v, mod)))
        u %= mod; v %= mod
        if trace is not None and a == 0 and trace.get('done') is None: trace['done'] = it + 1
        if trace is not None and b == 1 and trace.get('settled') is None: trace['settled'] = it + 1
    assert a == 0 and b == 1, (x, a, b)
    return v

def check(n_random=20000, seed=5, mod=P):
    """Every input converges within the 18 outer steps and matches Fermat; returns the worst
    number of outer steps any input needed."""
    rng = random.Random(seed)
    cases = [1, 2, 3, mod - 1, mod - 2, 2**255, 2**224, 2**96 - 1, (mod - 1) // 2, 2**64 - 1, 2**30 + 1] + [rng.randrange(1, mod) for _ in range(n_random)]
    worst = 0
    for x in cases:
        tr = {}
        r = inv(x, trace=tr, mod=mod)
        assert r == pow(x, mod - 2, mod), x
        worst = max(worst, tr['done'])
    return len(cases), worst


if __name__ == "__main__":
    n, worst = check()
    print("ok", n, "worst outer iterations to a == 0:", worst)
