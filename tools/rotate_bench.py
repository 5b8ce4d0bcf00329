"""The randomised block Hadamard rotation (rotate_kernel) against two yardsticks of the same process.

Per shape, one seeded float32 input on the device and, timed with HIP events on one stream, alternating in one process:
  decode_sum   flm_decode_sum_dev over the same N x L elements, in place: 8 bytes per element, HBM-bound, and in the
               library before the rotation was; run twice per round (decode_sum, decode_sum2), whose ratio is the A/A
               spread;
  encode_mask  flm_client_encode_mask_dev on the same batch (nearest-even, S seeds per client): what a client's masking
               costs, so what the rotation adds to it;
  fwd_h, inv_h flm_rotate_dev forward and inverse at log2_block h = 5, 8, 12 (one, two and three passes of the tile
               through its stages), not in place.
Before anything is timed, one row of each direction and block size is compared with the numpy restatement
(tests/rotate_cases.py) bit for bit.
Shapes: "agent" the agents' call (N = 1, L = 2^20, S = 25); "c3" the c3 batch (N = 1024 x L = 2^18, S = 41).
After --warmup untimed rounds, --reps rounds; medians and min..max in ms.  rotate's time over decode_sum's is per
element (the two move the same bytes); the margin is decode_sum's own max - min over its repetitions, as a share of
its median.  One JSON line on stdout.
"""
import argparse
import hashlib
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from flamingo_amd import MaskEngine  # noqa: E402

SHAPES = {"agent": (1, 1 << 20, 25), "c3": (1024, 1 << 18, 41)}
BLOCKS = (5, 8, 12)
F, CLIP = 16, 4.0
KEY = hashlib.sha256(b"rotate bench").digest()


def stats(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4),
            "reps": len(ms)}


def shape(eng, torch, name, reps, warmup):
    import rotate_cases as R
    N, L, S = SHAPES[name]
    g = np.random.Generator(np.random.PCG64(L + S))
    seeds = torch.from_numpy(g.integers(0, 256, (N * S, 32), dtype=np.uint8)).cuda()
    signs = np.where(g.integers(0, 2, N * S) == 1, 1, -1).astype(np.int8)
    seg = np.arange(N + 1, dtype=np.int64) * S
    gen = torch.Generator(device="cuda").manual_seed(L)
    x = torch.randn((N, L), generator=gen, device="cuda", dtype=torch.float32) * (CLIP / 3)
    y = torch.empty((N, L), dtype=torch.float32, device="cuda")         # L is a multiple of every block: L_rot = L
    words = torch.randint(-2 ** 31, 2 ** 31 - 1, (N * L,), generator=gen, device="cuda", dtype=torch.int64).to(torch.int32)
    masked = torch.empty((N, L), dtype=torch.int32, device="cuda")
    sb = torch.from_numpy(R.sign_words(KEY, L).view(np.int32).copy()).cuda()
    s = torch.cuda.Stream()

    row = x[N - 1].cpu().numpy()
    for h in BLOCKS:                                                     # the kernel's answers before its times
        assert eng.rotate_check(L, h) == L
        with torch.cuda.stream(s):
            eng.rotate_dev(x, y, L, h, sb, stream=s)
        s.synchronize()
        fw = y[N - 1].cpu().numpy()
        with torch.cuda.stream(s):
            eng.rotate_dev(x, y, L, h, sb, inverse=True, stream=s)
        s.synchronize()
        if fw.tobytes() != R.forward(row, KEY, h)[0].tobytes() or y[N - 1].cpu().numpy().tobytes() != R.inverse(row, KEY, h, L).tobytes():
            raise SystemExit(f"{name}: rotate_kernel differs from the restatement at h = {h}")

    legs = {"decode_sum": lambda: eng.decode_sum_dev(words, words.view(torch.float32), N * L, F, 1, stream=s),
            "encode_mask": lambda: eng.client_encode_mask_dev(seg, seeds, signs, masked, L, x, F, CLIP, stream=s)}
    for h in BLOCKS:
        legs[f"fwd_{h}"] = lambda h=h: eng.rotate_dev(x, y, L, h, sb, stream=s)
        legs[f"inv_{h}"] = lambda h=h: eng.rotate_dev(x, y, L, h, sb, inverse=True, stream=s)
    legs["decode_sum2"] = legs["decode_sum"]
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
    res = {"N": N, "L": L, "seeds_per_client": S, "bit_exact": True, **{k: stats(v) for k, v in t.items()},
           "bytes_moved": 8 * N * L,
           "aa_spread": round(med["decode_sum2"] / med["decode_sum"], 4),
           "decode_sum_margin": round((max(t["decode_sum"]) - min(t["decode_sum"])) / med["decode_sum"], 4),
           "decode_sum_GBps": round(8 * N * L / med["decode_sum"] / 1e6, 1)}
    for h in BLOCKS:
        for d in ("fwd", "inv"):
            k = f"{d}_{h}"
            res[k + "_over_decode_sum"] = round(med[k] / med["decode_sum"], 4)
            res[k + "_over_encode_mask"] = round(med[k] / med["encode_mask"], 4)
            res[k + "_GBps"] = round(8 * N * L / med[k] / 1e6, 1)
    return res


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="agent,c3")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    eng = MaskEngine(0)
    res = {"tool": "rotate_bench", "version": eng.lib.flm_version().decode()}
    for name in a.shapes.split(","):
        res[name] = shape(eng, torch, name, a.reps, a.warmup)
        torch.cuda.empty_cache()
    print(json.dumps(res))
    eng.close()


if __name__ == "__main__":
    main()
