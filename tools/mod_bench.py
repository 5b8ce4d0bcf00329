"""The decode modulo the field beside the worst-case packed decode it stands next to: decode_unpack_mod_kernel<2> and <4>
against decode_unpack_kernel<2> and <4>, in one process, at L = 2^22 parameters, with and without the near-wrap stats.

Both kernels read a word and write P floats per word, 4 + 4 P bytes, so the expected ratio is 1.  Legs per P, all on the
same summed words at a cohort both decodes admit (P = 2: (f, c, n) = (7, 1, 255); P = 4: (2, 1, 31)):
  old         flm_decode_unpack_dev
  mod         flm_decode_unpack_mod_dev, stats NULL
  mod_stats   flm_decode_unpack_mod_dev with stats (the call's 8-byte memset and the waves' atomics included)
A sample is the time between two events around --launches back-to-back calls of one leg, over the launches; the legs
alternate inside each round of repeats, so drift hits all of them alike.  After --warmup untimed rounds, --reps rounds;
min, median and max in microseconds per launch, and per P the ratios of the medians to `old` beside old's own max / min,
which is the noise floor of the run.  One JSON line on stdout.
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from flamingo_amd import MaskEngine  # noqa: E402

L_PARAMS = 1 << 22
PARAMS = {2: (7, 1.0, 255), 4: (2, 1.0, 31)}      # (f, c, n): the largest cohorts the worst-case rule admits


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--launches", type=int, default=20)
    a = ap.parse_args()
    eng = MaskEngine(0)
    s = torch.cuda.Stream()
    L = L_PARAMS
    g = np.random.Generator(np.random.PCG64(L))
    out = torch.empty(L, dtype=torch.float32, device="cuda")
    st = torch.zeros(2, dtype=torch.int32, device="cuda")
    legs = {}
    for P, (f, c, n) in PARAMS.items():
        words = torch.from_numpy(g.integers(0, 2 ** 32, L // P, dtype=np.uint64).astype(np.uint32).view(np.int32)).cuda()
        H = 1 << (32 // P - 1)
        legs[f"p{P}_old"] = lambda P=P, f=f, c=c, n=n, w=words: eng.decode_unpack_dev(w, out, L, f, c, P, n, stream=s)
        legs[f"p{P}_mod"] = lambda P=P, f=f, c=c, n=n, w=words: eng.decode_unpack_mod_dev(w, out, L, f, c, P, n, stream=s,
                                                                                       guard=H // 2)
        legs[f"p{P}_mod_stats"] = lambda P=P, f=f, c=c, n=n, w=words: eng.decode_unpack_mod_dev(
            w, out, L, f, c, P, n, stream=s, guard=H // 2, stats=st)
    t = {k: [] for k in legs}
    for r in range(a.warmup + a.reps):
        for k, fn in legs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            with torch.cuda.stream(s):
                e0.record(s)
                for _ in range(a.launches):
                    fn()
                e1.record(s)
            s.synchronize()
            if r >= a.warmup:
                t[k].append(e0.elapsed_time(e1) * 1e3 / a.launches)
    res = {"tool": "mod_bench", "version": eng.lib.flm_version().decode(), "L_params": L, "launches": a.launches, "reps": a.reps}
    for k, v in t.items():
        res[k] = {"min_us": round(min(v), 3), "median_us": round(statistics.median(v), 3), "max_us": round(max(v), 3)}
    for P in PARAMS:
        old = res[f"p{P}_old"]
        res[f"p{P}_old"]["max_over_min"] = round(old["max_us"] / old["min_us"], 4)
        res[f"p{P}_old"]["gb_per_s"] = round((4 + 4 * P) * (L // P) / (old["median_us"] * 1e-6) / 1e9, 1)
        for leg in ("mod", "mod_stats"):
            res[f"p{P}_{leg}"]["median_over_old"] = round(res[f"p{P}_{leg}"]["median_us"] / old["median_us"], 4)
            res[f"p{P}_{leg}"]["min_over_old_min"] = round(res[f"p{P}_{leg}"]["min_us"] / old["min_us"], 4)
    print(json.dumps(res))
    eng.close()


if __name__ == "__main__":
    main()
