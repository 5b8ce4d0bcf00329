"""The L2 clip (l2_sumsq_kernel + l2_factor_kernel, scale_rows_kernel, rotate_kernel<false, PHASES, true>) against the
rotation it rides in and the masking it precedes, in one process.

Per shape, one seeded float32 input on the device and, timed with HIP events on one stream, alternating:
  factors       flm_l2_factors_dev alone: reads 4 bytes per parameter, writes one partial per 4096;
  scale         flm_scale_rows_dev, not in place: 8 bytes per parameter;
  encode_mask   flm_client_encode_mask_dev on the same batch (nearest-even, S seeds per client): what a client's masking
                costs, so what the clip and the rotation add to it;
  fwd_h         flm_rotate_dev forward at log2_block h = 5, 8, 12, not in place: the unchanged kernel, 8 bytes per
                parameter;
  clip_h        flm_rotate_clip_dev on the same rows with the factors of `factors`: the same bytes and one multiply more;
  fused_h       flm_l2_factors_dev, then flm_rotate_clip_dev: the clip and the rotation as the agents run them;
  three_h       flm_l2_factors_dev, flm_scale_rows_dev, flm_rotate_dev: the same result without the fusion.
The radius is the median row norm (c3), or half the row's norm (agent), so rows on both sides of it are in the batch.
Before anything is timed every leg's result is compared with the numpy restatement (tests/l2_cases.py around
tests/rotate_cases.py) bit for bit on the first, second and last row, and the three-pass result with the fused one over
the whole batch.
Shapes: "agent" the agents' call (N = 1, L = 2^20, S = 25); "c3" the c3 batch (N = 1024 x L = 2^18, S = 41).
After --warmup untimed rounds, --reps rounds; medians and min..max in ms.  A leg's margin is its own (max - min) over
its median.  A table and one JSON line on stdout, and in --out when given.
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
KEY = hashlib.sha256(b"l2 bench").digest()


def stats(ms):
    med = statistics.median(ms)
    return {"median_ms": round(med, 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4),
            "margin": round((max(ms) - min(ms)) / med, 4), "reps": len(ms)}


def shape(eng, torch, name, reps, warmup):
    import l2_cases as l2
    import rotate_cases as R
    N, L, S = SHAPES[name]
    g = np.random.Generator(np.random.PCG64(L + S))
    seeds = torch.from_numpy(g.integers(0, 256, (N * S, 32), dtype=np.uint8)).cuda()
    signs = np.where(g.integers(0, 2, N * S) == 1, 1, -1).astype(np.int8)
    seg = np.arange(N + 1, dtype=np.int64) * S
    gen = torch.Generator(device="cuda").manual_seed(L)
    x = torch.randn((N, L), generator=gen, device="cuda", dtype=torch.float32) * (CLIP / 3)
    norms = torch.linalg.vector_norm(x.double(), dim=1)
    C = float(np.float32(norms.median().item() * (0.5 if N == 1 else 1.0)))
    y = torch.empty((N, L), dtype=torch.float32, device="cuda")         # L is a multiple of every block: L_rot = L
    y3 = torch.empty((N, L), dtype=torch.float32, device="cuda")
    mid = torch.empty((N, L), dtype=torch.float32, device="cuda")
    masked = torch.empty((N, L), dtype=torch.int32, device="cuda")
    sb = torch.from_numpy(R.sign_words(KEY, L).view(np.int32).copy()).cuda()
    work = torch.empty(eng.l2_clip_check(L, C, N), dtype=torch.float64, device="cuda")
    fac = torch.empty(N, dtype=torch.float32, device="cuda")
    ssq = torch.empty(N, dtype=torch.float64, device="cuda")
    s = torch.cuda.Stream()

    picks = sorted({0, min(1, N - 1), N - 1})
    rows = {i: x[i].cpu().numpy() for i in picks}
    want = {i: l2.clip(rows[i], C) for i in picks}
    with torch.cuda.stream(s):                                           # the kernels' answers before their times
        eng.l2_factors_dev(x, L, C, work, fac, ssq, stream=s)
        eng.scale_rows_dev(x, mid, L, fac, stream=s)
    s.synchronize()
    f_host, s_host = fac.cpu().numpy(), ssq.cpu().numpy()
    for i in picks:
        if f_host[i].tobytes() != want[i][1].tobytes() or s_host[i].tobytes() != want[i][2].tobytes():
            raise SystemExit(f"{name}: the factor or the sum of squares of row {i} differs from the restatement")
        if mid[i].cpu().numpy().tobytes() != want[i][0].tobytes():
            raise SystemExit(f"{name}: scale_rows_kernel differs from the restatement at row {i}")
    scaled_rows = int((f_host < 1.0).sum())
    for h in BLOCKS:
        assert eng.rotate_check(L, h) == L
        with torch.cuda.stream(s):
            eng.rotate_clip_dev(x, y, L, h, sb, fac, stream=s)
            eng.rotate_dev(mid, y3, L, h, sb, stream=s)
        s.synchronize()
        if not torch.equal(y.view(torch.int32), y3.view(torch.int32)):
            raise SystemExit(f"{name}: the fused rotation differs from scale + rotate at h = {h}")
        for i in picks:
            if y[i].cpu().numpy().tobytes() != R.forward(want[i][0], KEY, h)[0].tobytes():
                raise SystemExit(f"{name}: the fused rotation differs from the restatement at h = {h}, row {i}")
        with torch.cuda.stream(s):
            eng.rotate_dev(x, y3, L, h, sb, stream=s)
        s.synchronize()
        i = picks[-1]
        if y3[i].cpu().numpy().tobytes() != R.forward(rows[i], KEY, h)[0].tobytes():
            raise SystemExit(f"{name}: rotate_kernel differs from the restatement at h = {h}")

    def fused(h):
        eng.l2_factors_dev(x, L, C, work, fac, stream=s)
        eng.rotate_clip_dev(x, y, L, h, sb, fac, stream=s)

    def three(h):
        eng.l2_factors_dev(x, L, C, work, fac, stream=s)
        eng.scale_rows_dev(x, mid, L, fac, stream=s)
        eng.rotate_dev(mid, y, L, h, sb, stream=s)

    legs = {"factors": lambda: eng.l2_factors_dev(x, L, C, work, fac, stream=s),
            "scale": lambda: eng.scale_rows_dev(x, mid, L, fac, stream=s),
            "encode_mask": lambda: eng.client_encode_mask_dev(seg, seeds, signs, masked, L, x, F, CLIP, stream=s)}
    for h in BLOCKS:
        legs[f"fwd_{h}"] = lambda h=h: eng.rotate_dev(x, y, L, h, sb, stream=s)
        legs[f"clip_{h}"] = lambda h=h: eng.rotate_clip_dev(x, y, L, h, sb, fac, stream=s)
        legs[f"fused_{h}"] = lambda h=h: fused(h)
        legs[f"three_{h}"] = lambda h=h: three(h)
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
    res = {"N": N, "L": L, "seeds_per_client": S, "clip_norm": C, "rows_scaled": scaled_rows, "bit_exact": True,
           **{k: stats(v) for k, v in t.items()},
           "factors_GBps": round(4 * N * L / med["factors"] / 1e6, 1), "scale_GBps": round(8 * N * L / med["scale"] / 1e6, 1),
           "factors_over_encode_mask": round(med["factors"] / med["encode_mask"], 4)}
    for h in BLOCKS:
        res[f"fwd_{h}_GBps"] = round(8 * N * L / med[f"fwd_{h}"] / 1e6, 1)
        res[f"clip_{h}_GBps"] = round(8 * N * L / med[f"clip_{h}"] / 1e6, 1)
        res[f"clip_{h}_over_fwd"] = round(med[f"clip_{h}"] / med[f"fwd_{h}"], 4)
        res[f"factors_over_fwd_{h}"] = round(med["factors"] / med[f"fwd_{h}"], 4)
        res[f"fused_{h}_over_three"] = round(med[f"fused_{h}"] / med[f"three_{h}"], 4)
        res[f"fused_{h}_over_encode_mask"] = round(med[f"fused_{h}"] / med["encode_mask"], 4)
        res[f"fwd_{h}_over_encode_mask"] = round(med[f"fwd_{h}"] / med["encode_mask"], 4)
    return res


def table(res):
    out = []
    for name in SHAPES:
        if name not in res:
            continue
        r = res[name]
        out.append(f"{name}: N = {r['N']}, L = {r['L']}, S = {r['seeds_per_client']} seeds per client, clip_norm = "
                   f"{r['clip_norm']:.6g}, {r['rows_scaled']} of {r['N']} rows scaled")
        for k, v in r.items():
            if not isinstance(v, dict):
                continue
            extra = ""
            if k in ("factors", "scale"):
                extra = f"  {r[k + '_GBps']} GB/s"
            if k == "factors":
                extra += f", x{r['factors_over_encode_mask']} of encode_mask"
            kind, _, h = k.partition("_")
            if kind == "fwd" and h:
                extra = f"  {r[k + '_GBps']} GB/s, x{r[k + '_over_encode_mask']} of encode_mask; factors x{r['factors_over_' + k]} of it"
            if kind == "clip":
                extra = f"  {r[k + '_GBps']} GB/s, x{r[k + '_over_fwd']} of fwd_{h}"
            if kind == "fused":
                extra = f"  x{r[k + '_over_three']} of three_{h}, x{r[k + '_over_encode_mask']} of encode_mask"
            out.append(f"  {k:<12} {v['median_ms']:.4f} ({v['min_ms']:.4f}..{v['max_ms']:.4f})  margin {v['margin']}{extra}")
        out.append("")
    return "\n".join(out)


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="agent,c3")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    eng = MaskEngine(0)
    res = {"tool": "l2_bench", "version": eng.lib.flm_version().decode()}
    for name in a.shapes.split(","):
        res[name] = shape(eng, torch, name, a.reps, a.warmup)
        torch.cuda.empty_cache()
    text = table(res) + "\n" + json.dumps(res) + "\n"
    sys.stdout.write(text)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text)
    eng.close()


if __name__ == "__main__":
    main()
