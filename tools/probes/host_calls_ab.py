"""The batch crypto host-pointer calls alone, per-call wall time through ctypes with no Python packing
around them: flm_shamir_combine (T = 20, M = 4055), flm_shamir_deal and flm_aes_gcm_xor / _seal /
_open at one G = 8 rank's c5 share (M = 512 clients x 60 members, 32-byte shares, 16-byte AAD),
flm_ecdsa_verify (61 rows) and flm_feldman_verify (T = 22, M = 60, 60 rows) on random rows (every
row is refused early, so the lines are the call's host side plus a short launch).  Then the round-path
host calls: flm_client_mask and flm_client_encode_mask for one client (L = 2^20, 3 seeds) and for c2's
128 clients x 15 seeds x 16384 slots (the one-launch path), flm_decode_sum, flm_prg_expand (K = 8) and
flm_mask_accumulate at L = 2^20, flm_aggregate_unmask at the c2 shape.  Run once per library build
(FLM_LIB_PATH), as host_path_ab.py.  Median and min of 300 calls (100 for the ECDSA, Feldman and
many-client lines) after 20 warm ones."""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from flamingo_amd import MaskEngine  # noqa: E402
from flamingo_amd._lib import _u32p, p_f32, p_i8, p_i64, p_u8, p_u32  # noqa: E402

eng = MaskEngine(0)
lib, ctx = eng.lib, eng.ctx
g = np.random.Generator(np.random.PCG64(5))


def rnd(*shape):
    return g.integers(0, 256, shape, dtype=np.uint8)


def timed(name, fn, n=300):
    for _ in range(20):
        assert fn() == 0
    ts = []
    for _ in range(n):
        t = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t) * 1e3)
    print(f"{name}: median {np.median(ts):.4f} min {min(ts):.4f} ms", flush=True)


print(f"lib {os.environ.get('FLM_LIB_PATH', 'default')}", flush=True)
T, M = 20, 4055
sh, lam, so = rnd(T, M, 32), rnd(T, 32), np.zeros((M, 32), np.uint8)
timed("shamir_combine T=20 M=4055", lambda: lib.flm_shamir_combine(ctx, p_u8(sh), p_u8(lam), T, M, p_u8(so)))
M, C = 512, 60
co, xs, out = rnd(T, M, 32), np.arange(1, C + 1, dtype=np.uint32), np.zeros((C, M, 32), np.uint8)
timed("shamir_deal T=20 M=512 C=60", lambda: lib.flm_shamir_deal(ctx, p_u8(co), T, M, p_u32(xs), C, p_u8(out)))
n = M * C
k, nc, d, aad = rnd(n, 16), rnd(n, 16), rnd(n, 32), rnd(n, 16)
ct, pl, tg, ok = np.zeros((n, 32), np.uint8), np.zeros((n, 32), np.uint8), np.zeros((n, 16), np.uint8), np.zeros(n, np.uint8)
timed("aes_gcm_xor n=30720 len=32", lambda: lib.flm_aes_gcm_xor(ctx, p_u8(k), p_u8(nc), 16, p_u8(d), p_u8(ct), 32, n))
timed("aes_gcm_seal n=30720 len=32 aad=16",
      lambda: lib.flm_aes_gcm_seal(ctx, p_u8(k), p_u8(nc), 16, p_u8(aad), 16, p_u8(d), p_u8(ct), 32, p_u8(tg), n))
timed("aes_gcm_open n=30720 len=32 aad=16",
      lambda: lib.flm_aes_gcm_open(ctx, p_u8(k), p_u8(nc), 16, p_u8(aad), 16, p_u8(ct), p_u8(tg), p_u8(pl), 32, p_u8(ok), n))
assert ok.all() and (pl == d).all()
n = 61
pk, dg, sg, vok, fl = rnd(n, 64), rnd(n, 32), rnd(n, 64), np.zeros(n, np.uint8), np.zeros(n, np.uint32)
timed("ecdsa_verify n=61", lambda: lib.flm_ecdsa_verify(ctx, p_u8(pk), p_u8(dg), p_u8(sg), n, p_u8(vok), p_u32(fl)), 100)
T, M, n = 22, 60, 60
com, fx, fs = rnd(T, M, 64), np.full(n, 30, np.uint32), rnd(n, 32)
timed("feldman_verify T=22 M=60 n=60",
      lambda: lib.flm_feldman_verify(ctx, p_u8(com), T, M, None, p_u32(fx), 6, p_u8(fs), n, p_u8(vok[:n]), None,
                                     p_u32(fl[:n])), 100)

# ------------------------------------------------------------------ the round path
L = 1 << 20
for N, per, Lc, n_calls in ((1, 3, L, 300), (128, 15, 16384, 100)):
    K = N * per
    seg, sd, sg = np.arange(N + 1, dtype=np.int64) * per, rnd(K, 32), np.where(rnd(K) & 1, 1, -1).astype(np.int8)
    x, y = g.integers(0, 1 << 32, (N, Lc), dtype=np.uint32), np.zeros((N, Lc), np.uint32)
    xf, cl = g.standard_normal((N, Lc)).astype(np.float32), np.zeros(N, np.uint32)
    timed(f"client_mask N={N} K={K} L={Lc}",
          lambda: lib.flm_client_mask(ctx, p_u32(x), N, p_i64(seg), p_u8(sd), p_i8(sg), Lc, p_u32(y)), n_calls)
    timed(f"client_encode_mask N={N} K={K} L={Lc}",
          lambda: lib.flm_client_encode_mask(ctx, p_f32(xf), N, p_i64(seg), p_u8(sd), p_i8(sg), Lc, 16, 4.0, None, p_u32(y),
                                             p_u32(cl)), n_calls)
tot, mean = g.integers(0, 1 << 32, L, dtype=np.uint32), np.zeros(L, np.float32)
timed("decode_sum L=2^20", lambda: lib.flm_decode_sum(ctx, p_u32(tot), L, 16, 100, p_f32(mean)))
K = 8
sd, sg, ex = rnd(K, 32), np.ones(K, np.int8), np.zeros((K, L), np.uint32)
timed("prg_expand K=8 L=2^20", lambda: lib.flm_prg_expand(ctx, p_u8(sd), K, L, 0, p_u32(ex)))
acc = g.integers(0, 1 << 32, L, dtype=np.uint32)
timed("mask_accumulate K=8 L=2^20", lambda: lib.flm_mask_accumulate(ctx, p_u8(sd), p_i8(sg), K, p_u32(acc), L, 0))
N, K, Lc = 128, 1920, 16384                       # c2: 128 clients, 15 neighbours each
rows, sd, sg = g.integers(0, 1 << 32, (N, Lc), dtype=np.uint32), rnd(K, 32), np.where(rnd(K) & 1, 1, -1).astype(np.int8)
ptrs, total = (_u32p * N)(*[p_u32(r) for r in rows]), np.zeros(Lc, np.uint32)
timed("aggregate_unmask c2 N=128 K=1920 L=16384",
      lambda: lib.flm_aggregate_unmask(ctx, ptrs, N, p_u8(sd), p_i8(sg), K, Lc, p_u32(total)), 100)
eng.close()
