"""Distributed-DP binomial noise drawn inside client masking: what b coin flips per parameter cost.

Client-batch masking of float32 input at tools/pack_bench.py's shapes (c5: N = 1024 clients x 2^20 parameters,
S = 25 seeds each; agent: N = 1), for b = 0, 32, 64, 256 noise bits and P = 1, 2, 4 parameters per ring word,
nearest-even and stochastic, all through flm_client_encode_noise_mask_dev.  b = 0 dispatches the instantiations
without noise (encode_mask_kernel<P, STOCHASTIC, false>): the yardstick, timed in the same process.  b > 0 runs
encode_mask_kernel<P, STOCHASTIC, true>, which adds P ceil(b / 32) ChaCha blocks per word tile to the S seed blocks
and the E encoding blocks (E = P stochastic, 1 nearest: DESIGN.md section 5), so the block-count model of the ratio
is (S + E + P m) / (S + E).  Parameters: (f, c) = (7, 1) for P = 1 and 2, (2, 1) for P = 4; P = 4 has no headroom
for b = 256 at any (f, c) (2 (B + 128) > 255), so that leg is left out.
The legs alternate inside each round of repeats, so drift hits all of them alike.  After --warmup untimed rounds,
--reps rounds; medians and min..max in ms, the ratio to b = 0 beside the model's, one JSON line on stdout.
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
NOISE_BITS = (0, 32, 64, 256)


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
    noise = torch.from_numpy(g.integers(0, 256, (N, 32), dtype=np.uint8)).cuda()
    signs = np.where(g.integers(0, 2, N * S) == 1, 1, -1).astype(np.int8)
    seg = np.arange(N + 1, dtype=np.int64) * S
    gen = torch.Generator(device="cuda").manual_seed(L)
    x = torch.randn((N, L), generator=gen, device="cuda", dtype=torch.float32) * (1.0 / 3)
    out = torch.empty((N, L), dtype=torch.int32, device="cuda")     # P = 1's rows; the packed ones use its front
    s = torch.cuda.Stream()
    legs, model = {}, {}
    for P, (f, c) in PARAMS.items():
        o = out.view(-1)[:N * (L // P)].view(N, L // P)
        for mode, dd in (("nearest", None), ("stochastic", dither)):
            E = P if dd is not None else 1
            for b in NOISE_BITS:
                try:
                    eng.codec_check(f, c, 1, pack=P, noise_bits=b, L=L)
                except RuntimeError:
                    continue                                        # P = 4, b = 256: no headroom for one client
                k = f"p{P}_{mode}_b{b}"
                legs[k] = lambda f=f, c=c, dd=dd, P=P, o=o, b=b: eng.client_encode_noise_mask_dev(
                    seg, seeds, signs, o, L, x, f, c, P, dither_dev=dd, noise_bits=b, noise_dev=noise, stream=s)
                model[k] = (S + E + P * (-(-b // 32))) / (S + E)
    t = timed(torch, s, legs, reps, warmup)
    med = {k: statistics.median(v) for k, v in t.items()}
    res = {"N": N, "L_params": L, "seeds_per_client": S, **{k: stats(v) for k, v in t.items()}}
    for k in legs:
        res[k]["params_per_s"] = round(N * L / (med[k] * 1e-3), 1)
        res[k]["time_over_b0"] = round(med[k] / med[k.rsplit("_", 1)[0] + "_b0"], 4)
        res[k]["model_blocks_over_b0"] = round(model[k], 4)
    return res


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="c5,agent")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    eng = MaskEngine(0)
    res = {"tool": "dp_bench", "version": eng.lib.flm_version().decode(),
           "params": {f"p{P}": list(fc) for P, fc in PARAMS.items()}, "noise_bits": list(NOISE_BITS)}
    for part in a.parts.split(","):
        res["client_" + part] = client_shape(eng, torch, part, a.reps, a.warmup)
        torch.cuda.empty_cache()
    print(json.dumps(res))
    eng.close()


if __name__ == "__main__":
    main()
