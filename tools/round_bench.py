"""Conditional stochastic rounding's pass (round_sumsq_kernel + round_select_kernel) against the stochastic encode it
steers and the norm pass that reads the same rows, in one process.

Per shape, one seeded float32 input on the device and, timed with HIP events on one stream, alternating:
  select_A      flm_round_select_dev with A = 1, 4, 8 candidate dither seeds per row: reads 4 bytes per parameter once
                and runs A ChaCha blocks per 16 parameters;
  encode_mask   flm_client_encode_mask_dev on the same rows, stochastic rounding under the seeds select_4 chose, S mask
                seeds per client: S + 1 ChaCha blocks per 16 parameters (DESIGN.md section 5's block-count model);
  factors       flm_l2_factors_dev on the same rows: the one read of the row with next to no arithmetic.
The model printed beside each measured ratio: select_A costs the larger of `factors` (the read) and A / (S + 1) of
`encode_mask` (the blocks); `miss` is measured over modelled.
Before anything is timed the sums of the first and last row are compared with the restatement (tests/round_cases.py)
for the first and last candidate, the choices with its select, and the encoder's own words under the chosen seeds
(no mask seeds) with the sums the pass reported, over the whole batch.
Shapes: "agent" the agents' call (N = 1, L = 2^20, S = 25); "c5" the c5 client batch (N = 1024 x L = 2^20, S = 25).
After --warmup untimed rounds, --reps rounds; medians and min..max in ms.  A leg's margin is its own (max - min) over
its median.  A table and one JSON line on stdout, and in --out when given.
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from flamingo_amd import MaskEngine  # noqa: E402

SHAPES = {"agent": (1, 1 << 20, 25), "c5": (1024, 1 << 20, 25)}
ATTEMPTS = (1, 4, 8)
F, CLIP, TAIL = 16, 4.0, 1.0


def stats(ms):
    med = statistics.median(ms)
    return {"median_ms": round(med, 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4),
            "margin": round((max(ms) - min(ms)) / med, 4), "reps": len(ms)}


def shape(eng, torch, name, reps, warmup):
    import round_cases as RC
    N, L, S = SHAPES[name]
    g = np.random.Generator(np.random.PCG64(L + S + N))
    seeds = torch.from_numpy(g.integers(0, 256, (N * S, 32), dtype=np.uint8)).cuda()
    signs = np.where(g.integers(0, 2, N * S) == 1, 1, -1).astype(np.int8)
    seg = np.arange(N + 1, dtype=np.int64) * S
    cands_host = g.integers(0, 256, (N, max(ATTEMPTS), 32), dtype=np.uint8)
    cands = {A: torch.from_numpy(np.ascontiguousarray(cands_host[:, :A])).cuda() for A in ATTEMPTS}
    gen = torch.Generator(device="cuda").manual_seed(L + N)
    x = torch.randn((N, L), generator=gen, device="cuda", dtype=torch.float32) * (CLIP / 3)
    C = float(np.float32(torch.linalg.vector_norm(x.double(), dim=1).median().item()))
    max_sumsq = eng.round_bound(C, F, L, tail=TAIL)
    masked = torch.empty((N, L), dtype=torch.int32, device="cuda")
    sums = {A: torch.empty(N * A, dtype=torch.int64, device="cuda") for A in ATTEMPTS}
    dither = torch.empty((N, 32), dtype=torch.uint8, device="cuda")
    chosen = torch.empty(N, dtype=torch.int32, device="cuda")
    work = torch.empty(eng.l2_clip_check(L, C, N), dtype=torch.float64, device="cuda")
    fac = torch.empty(N, dtype=torch.float32, device="cuda")
    s = torch.cuda.Stream()

    # the kernels' answers before their times
    A = max(ATTEMPTS)
    with torch.cuda.stream(s):
        eng.round_select_dev(x, L, F, CLIP, cands[A], max_sumsq, sums[A], dither, chosen, stream=s)
    s.synchronize()
    got = sums[A].cpu().numpy().view(np.uint64).reshape(N, A)
    picks = chosen.cpu().numpy().view(np.uint32)
    for i in sorted({0, N - 1}):
        row = x[i].cpu().numpy()
        for a in (0, A - 1):
            if int(got[i, a]) != RC.sumsq(row, F, CLIP, bytes(cands_host[i, a])):
                raise SystemExit(f"{name}: the sum of squares of row {i}, candidate {a} differs from the restatement")
    if picks.tolist() != [RC.select(r, max_sumsq) for r in got.tolist()]:
        raise SystemExit(f"{name}: the choices differ from the restatement's")
    if dither.cpu().numpy().tobytes() != cands_host[np.arange(N), np.where(picks < A, picks, 0)].tobytes():
        raise SystemExit(f"{name}: the dither seeds are not the chosen candidates")
    none = torch.zeros((0, 32), dtype=torch.uint8, device="cuda")
    with torch.cuda.stream(s):                                           # the encoder's own words under those seeds
        eng.client_encode_mask_dev(np.zeros(N + 1, np.int64), none, np.zeros(0, np.int8), masked, L, x, F, CLIP,
                                   dither_dev=dither, stream=s)
        q = masked.to(torch.int64)
        enc = (q * q).sum(dim=1)                                         # L B^2 = 2^56: exact in int64
    s.synchronize()
    if enc.cpu().numpy().tolist() != [int(got[i, picks[i] if picks[i] < A else 0]) for i in range(N)]:
        raise SystemExit(f"{name}: the encoder's words do not square to the sums the pass reported")
    del q, enc
    with torch.cuda.stream(s):                                           # the seeds the timed encode rounds under
        eng.round_select_dev(x, L, F, CLIP, cands[4], max_sumsq, sums[4], dither, chosen, stream=s)
    s.synchronize()
    redrawn = int((chosen.cpu().numpy() != 0).sum())
    enc_dither = dither.clone()
    scratch = torch.empty((N, 32), dtype=torch.uint8, device="cuda")

    legs = {f"select_{A}": (lambda A=A: eng.round_select_dev(x, L, F, CLIP, cands[A], max_sumsq, sums[A], scratch, chosen,
                                                             stream=s)) for A in ATTEMPTS}
    legs["encode_mask"] = lambda: eng.client_encode_mask_dev(seg, seeds, signs, masked, L, x, F, CLIP, dither_dev=enc_dither,
                                                             stream=s)
    legs["factors"] = lambda: eng.l2_factors_dev(x, L, C, work, fac, stream=s)
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
    res = {"N": N, "L": L, "seeds_per_client": S, "frac_bits": F, "clip": CLIP, "clip_norm": C, "max_sumsq": max_sumsq,
           "rows_redrawn_of_4": redrawn, "bit_exact": True, **{k: stats(v) for k, v in t.items()},
           "factors_GBps": round(4 * N * L / med["factors"] / 1e6, 1)}
    for A in ATTEMPTS:
        k = f"select_{A}"
        model = max(med["factors"], A / (S + 1) * med["encode_mask"])
        res[k + "_GBps"] = round(4 * N * L / med[k] / 1e6, 1)
        res[k + "_Gblocks_per_s"] = round(A * N * L / 16 / med[k] / 1e6, 2)
        res[k + "_over_encode_mask"] = round(med[k] / med["encode_mask"], 4)
        res[k + "_over_factors"] = round(med[k] / med["factors"], 4)
        res[k + "_model_ms"] = round(model, 4)
        res[k + "_model_over_encode_mask"] = round(model / med["encode_mask"], 4)
        res[k + "_miss"] = round(med[k] / model, 4)
    res["encode_mask_Gblocks_per_s"] = round((S + 1) * N * L / 16 / med["encode_mask"] / 1e6, 2)
    res["select_4_costs_more_than_encode_mask"] = bool(med["select_4"] > med["encode_mask"])
    return res


def table(res):
    out = []
    for name in SHAPES:
        if name not in res:
            continue
        r = res[name]
        out.append(f"{name}: N = {r['N']}, L = {r['L']}, S = {r['seeds_per_client']} seeds per client, (f, c) = ({r['frac_bits']}, "
                   f"{r['clip']:g}), clip_norm = {r['clip_norm']:.6g}, max_sumsq = {r['max_sumsq']}, {r['rows_redrawn_of_4']} of "
                   f"{r['N']} rows past their first of 4 candidates")
        for k, v in r.items():
            if not isinstance(v, dict):
                continue
            extra = ""
            if k.startswith("select_"):
                extra = (f"  {r[k + '_GBps']} GB/s, {r[k + '_Gblocks_per_s']} G blocks/s, x{r[k + '_over_encode_mask']} of encode_mask "
                         f"(model x{r[k + '_model_over_encode_mask']}, miss x{r[k + '_miss']}), x{r[k + '_over_factors']} of factors")
            if k == "encode_mask":
                extra = f"  {r['encode_mask_Gblocks_per_s']} G blocks/s"
            if k == "factors":
                extra = f"  {r['factors_GBps']} GB/s"
            out.append(f"  {k:<12} {v['median_ms']:.4f} ({v['min_ms']:.4f}..{v['max_ms']:.4f})  margin {v['margin']}{extra}")
        out.append(f"  select_4 costs more than encode_mask: {r['select_4_costs_more_than_encode_mask']}")
        out.append("")
    return "\n".join(out)


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="agent,c5")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    eng = MaskEngine(0)
    res = {"tool": "round_bench", "version": eng.lib.flm_version().decode()}
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
