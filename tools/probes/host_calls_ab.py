"""The batch crypto host-pointer calls alone, per-call wall time through ctypes with no Python packing
around them: flm_shamir_combine (T = 20, M = 4055), flm_shamir_deal and flm_aes_gcm_xor / _seal /
_open at one G = 8 rank's c5 share (M = 512 clients x 60 members, 32-byte shares, 16-byte AAD),
flm_ecdsa_verify (61 rows) and flm_feldman_verify (T = 22, M = 60, 60 rows) on random rows (every
row is refused early, so the lines are the call's host side plus a short launch).  Run once per
library build (FLM_LIB_PATH), as host_path_ab.py.  Median and min of 300 calls (100 for the last
two) after 20 warm ones."""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from flamingo_amd import MaskEngine  # noqa: E402
from flamingo_amd._lib import p_u8, p_u32  # noqa: E402

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
eng.close()
