"""Discrete Gaussian noise shares sampled from a table inside client masking: what the table mode costs beside the
binomial mode that runs the same ChaCha blocks.

Client-batch masking of float32 input at tools/dp_bench.py's c5 shape (N = 1024 clients x 2^20 parameters, S = 25
seeds each), stochastic rounding, P = 1 and 2 parameters per ring word at (f, c) = (7, 1).  Legs: the table mode
(encode_gauss_mask_kernel<P, true>, flm_client_encode_gauss_mask_dev) at tau = 32, 128 and 512 with the discrete
Gaussian of sigma = tau / 10, beside the binomial mode at b = 64 (encode_mask_kernel<P, true, true>: the same two
ChaCha blocks per 16 parameters, popcounts where the table mode counts entries) and b = 0 (no noise).
The model printed beside each table leg is the b = 64 time plus the table probes at the LDS's conflict-free rate:
16 ceil(log2 T) ds_read_b64 per lane and unit (the bisection's last probe is left to the model's miss), one
wave-instruction of 64 x 8 bytes in 2 LDS cycles, every CU probing at once: N L ceil(log2 T) / 64 wave-instructions
x 2 cycles / (CUs x clock).  The probes of a wave go to 64 unrelated entries, so bank conflicts come on top: the miss
of the model is what they, the dependent-read latency and the occupancy of the kernel cost.
The legs alternate inside each round of repeats, so drift hits all of them alike.  After --warmup untimed rounds,
--reps rounds; medians and min..max in ms, one JSON line on stdout.
"""
import argparse
import json
import math
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from flamingo_amd import MaskEngine, dgauss  # noqa: E402

F, C = 7, 1.0
SHAPE = (1024, 1 << 20, 25)
TAILS = (32, 128, 512)
PACKS = (1, 2)
LDS_CYCLES_PER_READ = 2.0       # one conflict-free ds_read_b64 wave-instruction


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


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--clients", type=int, default=SHAPE[0])
    ap.add_argument("--clock_ghz", type=float, default=2.4)
    a = ap.parse_args()
    eng = MaskEngine(0)
    N, L, S = a.clients, SHAPE[1], SHAPE[2]
    cus = eng.cu_count()
    g = np.random.Generator(np.random.PCG64(L + S + N))
    seeds = torch.from_numpy(g.integers(0, 256, (N * S, 32), dtype=np.uint8)).cuda()
    dither = torch.from_numpy(g.integers(0, 256, (N, 32), dtype=np.uint8)).cuda()
    noise = torch.from_numpy(g.integers(0, 256, (N, 32), dtype=np.uint8)).cuda()
    signs = np.where(g.integers(0, 2, N * S) == 1, 1, -1).astype(np.int8)
    seg = np.arange(N + 1, dtype=np.int64) * S
    gen = torch.Generator(device="cuda").manual_seed(L)
    x = torch.randn((N, L), generator=gen, device="cuda", dtype=torch.float32) * (1.0 / 3)
    out = torch.empty((N, L), dtype=torch.int32, device="cuda")     # P = 1's rows; the packed ones use its front
    tables = {tau: torch.from_numpy(dgauss.table(tau / 10.0, tau).view(np.int64).copy()).cuda() for tau in TAILS}
    s = torch.cuda.Stream()
    legs = {}
    for P in PACKS:
        o = out.view(-1)[:N * (L // P)].view(N, L // P)
        for b in (0, 64):
            legs[f"p{P}_binomial_b{b}"] = lambda P=P, o=o, b=b: eng.client_encode_noise_mask_dev(
                seg, seeds, signs, o, L, x, F, C, P, dither_dev=dither, noise_bits=b, noise_dev=noise, stream=s)
        for tau in TAILS:
            eng.codec_check_gauss(F, C, tau, 1, pack=P, L=L)
            legs[f"p{P}_table_tau{tau}"] = lambda P=P, o=o, tau=tau: eng.client_encode_gauss_mask_dev(
                seg, seeds, signs, o, L, x, F, C, tables[tau], noise, pack=P, dither_dev=dither, stream=s)
    t = timed(torch, s, legs, a.reps, a.warmup)
    med = {k: statistics.median(v) for k, v in t.items()}
    res = {"tool": "dgauss_bench", "version": eng.lib.flm_version().decode(), "N": N, "L_params": L, "seeds_per_client": S,
           "frac_bits": F, "clip": C, "rounding": "stochastic", "cus": cus, "model_clock_ghz": a.clock_ghz,
           **{k: stats(v) for k, v in t.items()}}
    for k in legs:
        res[k]["params_per_s"] = round(N * L / (med[k] * 1e-3), 1)
        res[k]["time_over_b64"] = round(med[k] / med[k.split("_")[0] + "_binomial_b64"], 4)
        if "_table_tau" in k:
            T = 2 * int(k.rsplit("tau", 1)[1])
            probes_ms = N * L * math.ceil(math.log2(T)) / 64 * LDS_CYCLES_PER_READ / (cus * a.clock_ghz * 1e9) * 1e3
            model = med[k.split("_")[0] + "_binomial_b64"] + probes_ms
            res[k].update(model_ms=round(model, 4), model_probes_ms=round(probes_ms, 4),
                          measured_over_model=round(med[k] / model, 4))
    print(json.dumps(res))
    eng.close()


if __name__ == "__main__":
    main()
