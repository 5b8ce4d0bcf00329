"""Client masking of float updates: the fixed-point encoding fused into the masking kernel against encoding first.

Per shape, one seeded float32 input on the device, S seeds per client (the neighbour graph's degree
2 o log2(n) plus the self mask), and four legs timed with HIP events on one stream, alternating in one process:
  a   flm_client_mask_dev on the pre-encoded uint32 input (the kernel as it was; run twice per round: a, a2,
      whose ratio is the A/A spread);
  b   a torch encode pass (nan_to_num, clamp, scale, round, to int32) followed by a: what a caller does without
      the codec;
  c   flm_client_encode_mask_dev, nearest-even;
  d   flm_client_encode_mask_dev, stochastic (one dither block per lane more).
Before anything is timed, c's bytes are compared with a's on torch's encoding of the same input.
Shapes: "c5" N = 1024 clients x L = 2^20 at c5's S = 25; "c3" N = 1024 x L = 2^18 at S = 41; "agent" the
agents' one-client host-pointer call (N = 1, L = 2^20, S = 25): client_encode_mask against client_mask, wall time.
After --warmup untimed rounds, --reps rounds; medians and min..max in ms, one JSON line on stdout.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from flamingo_amd import MaskEngine  # noqa: E402

SHAPES = {"c5": (1024, 1 << 20, 25), "c3": (1024, 1 << 18, 41)}
F, CLIP = 16, 4.0


def stats(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4),
            "reps": len(ms)}


def device_shape(eng, torch, name, reps, warmup):
    N, L, S = SHAPES[name]
    g = np.random.Generator(np.random.PCG64(L + S))
    seeds = torch.from_numpy(g.integers(0, 256, (N * S, 32), dtype=np.uint8)).cuda()
    dither = torch.from_numpy(g.integers(0, 256, (N, 32), dtype=np.uint8)).cuda()
    signs = np.where(g.integers(0, 2, N * S) == 1, 1, -1).astype(np.int8)
    seg = np.arange(N + 1, dtype=np.int64) * S
    gen = torch.Generator(device="cuda").manual_seed(L)
    x = torch.randn((N, L), generator=gen, device="cuda", dtype=torch.float32) * (CLIP / 3)
    out = torch.empty((N, L), dtype=torch.int32, device="cuda")
    ref = torch.empty((N, L), dtype=torch.int32, device="cuda")
    s = torch.cuda.Stream()

    def encode():
        return torch.round(torch.clamp(torch.nan_to_num(x, nan=0.0), -CLIP, CLIP) * float(1 << F)).to(torch.int32)

    q = encode()
    legs = {
        "a": lambda: eng.client_mask_dev(seg, seeds, signs, ref, L, x=q, stream=s),
        "a2": lambda: eng.client_mask_dev(seg, seeds, signs, ref, L, x=q, stream=s),
        "b": lambda: eng.client_mask_dev(seg, seeds, signs, ref, L, x=encode(), stream=s),
        "c": lambda: eng.client_encode_mask_dev(seg, seeds, signs, out, L, x, F, CLIP, stream=s),
        "d": lambda: eng.client_encode_mask_dev(seg, seeds, signs, out, L, x, F, CLIP, dither_dev=dither, stream=s),
    }
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        legs["a"]()
        legs["c"]()
    s.synchronize()
    if not torch.equal(out, ref):
        raise SystemExit(f"{name}: the fused kernel differs from masking the encoded input")
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
    med = {k: statistics.median(v) for k, v in t.items()}
    return {"N": N, "L": L, "seeds_per_client": S, "frac_bits": F, "clip": CLIP, "byte_exact": True,
            **{k: stats(v) for k, v in t.items()},
            "aa_spread": round(med["a2"] / med["a"], 4), "c_over_a": round(med["c"] / med["a"], 4),
            "d_over_a": round(med["d"] / med["a"], 4), "c_over_b": round(med["c"] / med["b"], 4),
            "expected_c_over_a": round(1 + 6 / (61 * S), 4), "expected_d_over_a": round((S + 1) / S, 4)}


def agent_shape(eng, reps, warmup, L=1 << 20, S=25):
    g = np.random.Generator(np.random.PCG64(7))
    seeds = g.integers(0, 256, (S, 32), dtype=np.uint8)
    signs = np.where(g.integers(0, 2, S) == 1, 1, -1).astype(np.int8)
    seg = np.array([0, S], np.int64)
    x = (g.standard_normal((1, L)) * (CLIP / 3)).astype(np.float32)
    q = np.rint(np.clip(x, -CLIP, CLIP) * np.float32(1 << F)).astype(np.int32).view(np.uint32)
    dither = g.integers(0, 256, (1, 32), dtype=np.uint8)
    legs = {
        "client_mask": lambda: eng.client_mask(seg, seeds, signs, L, x=q),
        "numpy_encode_then_client_mask": lambda: eng.client_mask(
            seg, seeds, signs, L, x=np.rint(np.clip(np.nan_to_num(x), -CLIP, CLIP) * np.float32(1 << F)).astype(np.int32).view(np.uint32)),
        "client_encode_mask": lambda: eng.client_encode_mask(seg, seeds, signs, L, x, F, CLIP),
        "client_encode_mask_stochastic": lambda: eng.client_encode_mask(seg, seeds, signs, L, x, F, CLIP, dither=dither),
    }
    if not np.array_equal(legs["client_mask"](), legs["client_encode_mask"]()):
        raise SystemExit("agent: the fused call differs from masking the encoded input")
    t = {k: [] for k in legs}
    for r in range(warmup + reps):
        for k, fn in legs.items():
            t0 = time.perf_counter()
            fn()
            if r >= warmup:
                t[k].append((time.perf_counter() - t0) * 1e3)
    return {"N": 1, "L": L, "seeds_per_client": S, "wall": True, "byte_exact": True, **{k: stats(v) for k, v in t.items()}}


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="c5,c3,agent")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    eng = MaskEngine(0)
    res = {"tool": "codec_bench", "version": eng.lib.flm_version().decode()}
    for name in a.shapes.split(","):
        res[name] = agent_shape(eng, a.reps, a.warmup) if name == "agent" else device_shape(eng, torch, name, a.reps,
                                                                                            a.warmup)
        torch.cuda.empty_cache()
    print(json.dumps(res))
    eng.close()


if __name__ == "__main__":
    main()
