"""Dealing and sealing the clients' m_i shares at BASELINE c5's shape: M clients, the c5 committee
(C = params.committee_size members, threshold T = int(params.fraction * C)), 32-byte shares -- the
whole iteration (M = 4096) or one G = 8 rank's share of it (--ranks 8: M = 512).

Timed in one process, on the same seeded inputs:
  host  the per-client host path: seeds.shamir_share per client + crypto.aes_gcm_encrypt per
        share, on one core (the path of protocol.configure(gpu_deal=False));
  gpu   MaskEngine.shamir_deal_wire + aes_gcm_xor_wire, the host-pointer calls (copies included);
  dev   shamir_deal_dev + aes_gcm_xor_dev on device-resident tensors, HIP events over the pair.
The gpu and dev outputs are compared with the host path's byte for byte before anything is
reported; a mismatch is an error.  After --warmup untimed runs each leg runs --reps times (the host
leg --host-reps times: it takes seconds); the line gives the median and the min..max spread in ms.
One JSON line on stdout.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from flamingo_amd import MaskEngine, crypto as C, params as P  # noqa: E402
from flamingo_amd.abides.flamingo.seeds import P256_N, shamir_share  # noqa: E402


class _Coeffs:
    """randrange() that hands out a fixed list: shamir_share then uses our polynomial."""

    def __init__(self, vals):
        self.vals = iter(vals)

    def randrange(self, n):
        return next(self.vals)


def stats(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4),
            "reps": len(ms)}


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--clients", type=int, default=4096)
    ap.add_argument("--ranks", type=int, default=1, help="time one rank's share: clients / ranks")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    M, Cn = a.clients // a.ranks, P.committee_size
    T = max(1, int(P.fraction * Cn))
    g = np.random.Generator(np.random.PCG64(4096))
    coeffs = g.integers(0, 256, (T, M, 32), dtype=np.uint8)          # term 0: m_i, any 32 bytes
    keys = g.integers(0, 256, (M, Cn, 16), dtype=np.uint8)
    nonces = g.integers(0, 256, (M, Cn, 16), dtype=np.uint8)
    xs = np.arange(1, Cn + 1, dtype=np.uint32)
    ints = [[int.from_bytes(coeffs[j, i].tobytes(), "big") for j in range(T)] for i in range(M)]
    kb, nb = keys.tobytes(), nonces.tobytes()

    def host():
        out = []
        for i in range(M):
            pts = shamir_share(ints[i][0], T, Cn, P256_N, rng=_Coeffs(v % P256_N for v in ints[i][1:]))
            for c, (_, y) in enumerate(pts):
                o = 16 * (i * Cn + c)
                out.append(C.aes_gcm_encrypt(kb[o:o + 16], y.to_bytes(32, "big"), nb[o:o + 16])[0])
        return b"".join(out)

    eng = MaskEngine(0)
    k2, n2 = keys.reshape(M * Cn, 16), nonces.reshape(M * Cn, 16)

    def gpu():
        shares = eng.shamir_deal_wire(coeffs, xs)                                          # (C, M, 32)
        return eng.aes_gcm_xor_wire(k2, n2, np.ascontiguousarray(shares.transpose(1, 0, 2)).reshape(M * Cn, 32))

    s = torch.cuda.Stream()
    d_co, d_xs = torch.from_numpy(coeffs).cuda(), torch.from_numpy(xs.view(np.int32)).cuda()
    # the sealing reads the shares where the dealing wrote them (point-major): keys and nonces in that order
    d_k = torch.from_numpy(np.ascontiguousarray(keys.transpose(1, 0, 2)).reshape(Cn * M, 16)).cuda()
    d_n = torch.from_numpy(np.ascontiguousarray(nonces.transpose(1, 0, 2)).reshape(Cn * M, 16)).cuda()
    d_sh = torch.empty((Cn, M, 32), dtype=torch.uint8, device="cuda")
    d_ct = torch.empty((Cn * M, 32), dtype=torch.uint8, device="cuda")

    def dev():
        e0, e1, e2 = (torch.cuda.Event(enable_timing=True) for _ in range(3))
        e0.record(s)
        eng.shamir_deal_dev(d_co, d_xs, d_sh, stream=s)
        e1.record(s)
        eng.aes_gcm_xor_dev(d_k, d_n, d_sh.view(Cn * M, 32), out=d_ct, stream=s)
        e2.record(s)
        s.synchronize()
        return e0.elapsed_time(e1), e1.elapsed_time(e2)

    def wall(fn):
        t0 = time.perf_counter()
        r = fn()
        return r, (time.perf_counter() - t0) * 1e3

    want, t_first = wall(host)
    want = np.frombuffer(want, np.uint8).reshape(M, Cn, 32)
    if not np.array_equal(gpu().reshape(M, Cn, 32), want):
        raise SystemExit("host-pointer GPU path differs from the host path")
    dev()
    if not np.array_equal(d_ct.cpu().numpy().reshape(Cn, M, 32).transpose(1, 0, 2), want):
        raise SystemExit("device GPU path differs from the host path")
    for _ in range(a.warmup):
        gpu()
        dev()
    t_host = [t_first] + [wall(host)[1] for _ in range(a.host_reps - 1)]
    t_gpu = [wall(gpu)[1] for _ in range(a.reps)]
    t_dev = [dev() for _ in range(a.reps)]
    print(json.dumps({
        "tool": "deal_bench", "clients": M, "ranks": a.ranks, "committee": Cn, "threshold": T, "share_bytes": 32,
        "shares": M * Cn, "byte_exact": True,
        "host_one_core": stats(t_host), "gpu_host_pointer_calls": stats(t_gpu),
        "dev_shamir_deal": stats([d[0] for d in t_dev]), "dev_aes_gcm_xor": stats([d[1] for d in t_dev]),
        "dev_both": stats([d[0] + d[1] for d in t_dev]), "version": eng.lib.flm_version().decode()}))
    eng.close()


if __name__ == "__main__":
    main()
