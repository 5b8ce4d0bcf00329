"""The packed codec against the unpacked one at the same parameter count: P = 1 (client_encode_mask, decode_sum:
the code as it was), 2 and 4 parameters per ring word, timed in one process with HIP events on one stream.

  client   client masking of float32 input, nearest-even and stochastic, at the c5 batch shape (N = 1024 clients x
           2^20 parameters, S = 25 seeds each) and at the agents' one-client shape (N = 1, 2^20 parameters, S = 25):
           flm_client_encode_mask_dev (P = 1) against flm_client_encode_pack_mask_dev; ms and parameters/s;
  round    the server's round, n rows of ceil(L / P) words plus K masks (flm_aggregate_unmask_dev), then the
           decode (flm_decode_sum_dev in place, flm_decode_unpack_dev); n = 31 rows, the largest cohort P = 4
           admits at (2, 1), so that all three run the same cohort, and n = 255 for P = 1 and 2;
  decode   the decode alone at 2^24 parameters, in GB/s of words read plus floats written.
Parameters: (f, c) = (7, 1) for P = 1 and 2, (2, 1) for P = 4 (8-bit fields hold nothing finer for even one client).
The legs alternate inside each round of repeats, so drift hits all of them alike.  After --warmup untimed rounds,
--reps rounds; medians and min..max in ms and the ratios to P = 1, one JSON line on stdout.
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from flamingo_amd import MaskEngine  # noqa: E402

PARAMS = {1: (7, 1.0), 2: (7, 1.0), 4: (2, 1.0)}
CLIENT_SHAPES = {"c5": (1024, 1 << 20, 25), "agent": (1, 1 << 20, 25)}
ROUND_L, ROUND_COHORTS = 1 << 20, {31: (1, 2, 4), 255: (1, 2)}
DECODE_L = 1 << 24


def stats(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4),
            "reps": len(ms)}


def timed(torch, s, legs, reps, warmup):
    t = {k: [] for k in legs}
    for r in range(warmup + reps):
        for k, fn in legs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            with torch.cuda.stream(s):
                e0.record(s)
                fn()
                e1.record(s)
            s.synchronize()
            if r >= warmup:
                t[k].append(e0.elapsed_time(e1))
    return t


def client_shape(eng, torch, name, reps, warmup):
    N, L, S = CLIENT_SHAPES[name]
    g = np.random.Generator(np.random.PCG64(L + S + N))
    seeds = torch.from_numpy(g.integers(0, 256, (N * S, 32), dtype=np.uint8)).cuda()
    dither = torch.from_numpy(g.integers(0, 256, (N, 32), dtype=np.uint8)).cuda()
    signs = np.where(g.integers(0, 2, N * S) == 1, 1, -1).astype(np.int8)
    seg = np.arange(N + 1, dtype=np.int64) * S
    gen = torch.Generator(device="cuda").manual_seed(L)
    x = torch.randn((N, L), generator=gen, device="cuda", dtype=torch.float32) * (1.0 / 3)
    out = torch.empty((N, L), dtype=torch.int32, device="cuda")     # P = 1's rows; the packed ones use its front
    s = torch.cuda.Stream()
    legs = {}
    for P, (f, c) in PARAMS.items():
        for mode, dd in (("nearest", None), ("stochastic", dither)):
            if P == 1:
                legs[f"p1_{mode}"] = lambda f=f, c=c, dd=dd: eng.client_encode_mask_dev(
                    seg, seeds, signs, out, L, x, f, c, dither_dev=dd, stream=s)
            else:
                o = out.view(-1)[:N * (L // P)].view(N, L // P)
                legs[f"p{P}_{mode}"] = lambda f=f, c=c, dd=dd, P=P, o=o: eng.client_encode_pack_mask_dev(
                    seg, seeds, signs, o, L, x, f, c, P, dither_dev=dd, stream=s)
    t = timed(torch, s, legs, reps, warmup)
    med = {k: statistics.median(v) for k, v in t.items()}
    res = {"N": N, "L_params": L, "seeds_per_client": S, **{k: stats(v) for k, v in t.items()}}
    for k in legs:
        res[k]["params_per_s"] = round(N * L / (med[k] * 1e-3), 1)
        res[k]["time_over_p1"] = round(med[k] / med["p1_" + k.split("_")[1]], 4)
    return res


def round_shape(eng, torch, n, packs, reps, warmup):
    L = ROUND_L
    K = n + n // 4                      # the survivors' self masks and a quarter as many dropped-pair masks
    g = np.random.Generator(np.random.PCG64(n))
    seeds = torch.from_numpy(g.integers(0, 256, (K, 32), dtype=np.uint8)).cuda()
    signs = torch.from_numpy(np.where(g.integers(0, 2, K) == 1, 1, -1).astype(np.int8)).cuda()
    gen = torch.Generator(device="cuda").manual_seed(n)
    rows = torch.randint(-2 ** 31, 2 ** 31, (n, L), generator=gen, device="cuda", dtype=torch.int64).to(torch.int32)
    s = torch.cuda.Stream()
    legs, bufs = {}, {}
    for P in packs:
        f, c = PARAMS[P]
        Lw = L // P
        total = torch.empty(Lw, dtype=torch.int32, device="cuda")
        mean = torch.empty(L, dtype=torch.float32, device="cuda")
        bufs[P] = (total, mean)
        r = rows[:, :Lw]                # the same rows, the first Lw words of each: pitch L

        def leg(P=P, f=f, c=c, Lw=Lw, total=total, mean=mean, r=r):
            eng.aggregate_unmask_dev(r, seeds, signs, total, L=Lw, stream=s)
            if P == 1:
                eng.decode_sum_dev(total, total.view(torch.float32), L, f, n, stream=s)
            else:
                eng.decode_unpack_dev(total, mean, L, f, c, P, n, stream=s)
        legs[f"p{P}"] = leg
    t = timed(torch, s, legs, reps, warmup)
    med = {k: statistics.median(v) for k, v in t.items()}
    res = {"rows": n, "L_params": L, "masks": K, **{k: stats(v) for k, v in t.items()}}
    for k in legs:
        res[k]["time_over_p1"] = round(med[k] / med["p1"], 4)
    return res


def decode_alone(eng, torch, reps, warmup):
    L = DECODE_L
    gen = torch.Generator(device="cuda").manual_seed(3)
    words = torch.randint(-2 ** 31, 2 ** 31, (L,), generator=gen, device="cuda", dtype=torch.int64).to(torch.int32)
    mean = torch.empty(L, dtype=torch.float32, device="cuda")
    s = torch.cuda.Stream()
    legs = {"p1": lambda: eng.decode_sum_dev(words, mean, L, 7, 31, stream=s)}
    for P in (2, 4):
        f, c = PARAMS[P]
        legs[f"p{P}"] = lambda P=P, f=f, c=c: eng.decode_unpack_dev(words, mean, L, f, c, P, 31, stream=s)
    t = timed(torch, s, legs, reps, warmup)
    med = {k: statistics.median(v) for k, v in t.items()}
    res = {"L_params": L, **{k: stats(v) for k, v in t.items()}}
    for k in legs:
        P = int(k[1:])
        res[k]["GB_per_s"] = round((L // P + L) * 4 / (med[k] * 1e-3) / 1e9, 1)
        res[k]["time_over_p1"] = round(med[k] / med["p1"], 4)
    return res


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="c5,agent,round,decode")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    eng = MaskEngine(0)
    res = {"tool": "pack_bench", "version": eng.lib.flm_version().decode(),
           "params": {f"p{P}": list(fc) for P, fc in PARAMS.items()}}
    for part in a.parts.split(","):
        if part in CLIENT_SHAPES:
            res["client_" + part] = client_shape(eng, torch, part, a.reps, a.warmup)
        elif part == "round":
            for n, packs in ROUND_COHORTS.items():
                res[f"round_n{n}"] = round_shape(eng, torch, n, packs, a.reps, a.warmup)
        elif part == "decode":
            res["decode"] = decode_alone(eng, torch, a.reps, a.warmup)
        torch.cuda.empty_cache()
    print(json.dumps(res))
    eng.close()


if __name__ == "__main__":
    main()
