"""ECDSA verification on the GPU against the host loop, at the sizes the protocol meets: 61 rows (one
committee member's DEC at committee size 60: the server's signature + 60 members'), 3,660 (every
member's check of an iteration in one call), 4,096 and 245,760.

Rows are OpenSSL signatures (crypto.ecdsa_sign) over distinct messages under distinct keys, every
eighth one tampered; a pool of --pool signed rows is tiled to the larger sizes.  Timed in one process:
  host  crypto.ecdsa_verify row by row (OpenSSL through ctypes, SHA-256 of the message included),
        on at most --host-rows rows; the line gives the time per row and the time for all n rows
        at that rate;
  list  MaskEngine.ecdsa_verify, the call the agents make (hashing and packing included), n <= 4,096;
  gpu   MaskEngine.ecdsa_verify_wire, the host-pointer call on packed arrays (copies included);
  dev   ecdsa_verify_dev on device-resident tensors, HIP events around the bare kernel.
Every GPU verdict is compared with the host loop's (on the pool) before anything is reported; a
mismatch is an error.  Median and min..max over --reps runs after --warmup untimed ones, in ms.
One JSON line per size on stdout.
"""
import argparse
import hashlib
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from flamingo_amd import MaskEngine, crypto as C  # noqa: E402


def stats(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4),
            "reps": len(ms)}


def wall(fn):
    t0 = time.perf_counter()
    r = fn()
    return r, (time.perf_counter() - t0) * 1e3


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="61,3660,4096,245760")
    ap.add_argument("--pool", type=int, default=4096)
    ap.add_argument("--host-rows", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    sizes = [int(s) for s in a.sizes.split(",")]
    pool = min(a.pool, max(sizes))
    keys = [C.keygen(b"bench%d" % i) for i in range(pool)]
    msgs = [b"[%d, %d, %d]" % (i, 2 * i + 1, 3 * i + 7) for i in range(pool)]
    sigs = [C.ecdsa_sign(d, Q, m) for (d, Q), m in zip(keys, msgs)]
    for i in range(7, pool, 8):
        sigs[i] = sigs[i][:50] + bytes([sigs[i][50] ^ 0x10]) + sigs[i][51:]
    pubs = [Q for _, Q in keys]
    want_pool = np.array([C.ecdsa_verify(p, m, s) for p, m, s in zip(pubs, msgs, sigs)])
    assert int(want_pool.sum()) == pool - len(range(7, pool, 8))
    pk_pool = C.points_to_wire(pubs)
    dg_pool = np.frombuffer(b"".join(hashlib.sha256(m).digest() for m in msgs), np.uint8).reshape(pool, 32)
    sg_pool = np.frombuffer(b"".join(sigs), np.uint8).reshape(pool, 64)
    eng = MaskEngine(0)
    s = torch.cuda.Stream()
    for n in sizes:
        idx = np.arange(n) % pool
        pk, dg, sg, want = pk_pool[idx], dg_pool[idx], sg_pool[idx], want_pool[idx]
        h = min(n, a.host_rows)
        hp, hm, hs = [pubs[i] for i in idx[:h]], [msgs[i] for i in idx[:h]], [sigs[i] for i in idx[:h]]

        def host():
            return [C.ecdsa_verify(p, m, g) for p, m, g in zip(hp, hm, hs)]

        d_pk, d_dg, d_sg = (torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in (pk, dg, sg))
        d_ok = torch.zeros(n, dtype=torch.uint8, device="cuda")
        d_fl = torch.zeros(n, dtype=torch.int32, device="cuda")

        def dev():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(s)
            eng.ecdsa_verify_dev(d_pk, d_dg, d_sg, d_ok, d_fl, stream=s)
            e1.record(s)
            s.synchronize()
            return e0.elapsed_time(e1)

        got, _ = eng.ecdsa_verify_wire(pk, dg, sg)
        if not np.array_equal(got, want):
            raise SystemExit(f"n={n}: the host-pointer GPU verdicts differ from the host loop's")
        dev()
        if not np.array_equal(d_ok.cpu().numpy().astype(bool), want):
            raise SystemExit(f"n={n}: the device-form verdicts differ from the host loop's")
        if host() != list(want[:h]):
            raise SystemExit(f"n={n}: the host loop disagrees with itself")
        for _ in range(a.warmup):
            eng.ecdsa_verify_wire(pk, dg, sg)
            dev()
        t_host = [wall(host)[1] for _ in range(a.host_reps)]
        t_gpu = [wall(lambda: eng.ecdsa_verify_wire(pk, dg, sg))[1] for _ in range(a.reps)]
        t_dev = [dev() for _ in range(a.reps)]
        line = {"tool": "ecdsa_verify_bench", "n": n, "valid": int(want.sum()), "verdicts_match": True,
                "host_rows_timed": h, "host_loop": stats(t_host),
                "host_us_per_row": round(statistics.median(t_host) * 1e3 / h, 2),
                "host_loop_all_rows_ms": round(statistics.median(t_host) * n / h, 3),
                "gpu_host_pointer_call": stats(t_gpu), "dev_kernel": stats(t_dev)}
        if n <= 4096:
            if eng.ecdsa_verify(hp, hm, hs) != list(want):
                raise SystemExit(f"n={n}: MaskEngine.ecdsa_verify differs from the host loop")
            line["gpu_list_call"] = stats([wall(lambda: eng.ecdsa_verify(hp, hm, hs))[1] for _ in range(a.reps)])
        line["version"] = eng.lib.flm_version().decode()
        print(json.dumps(line), flush=True)
    eng.close()


if __name__ == "__main__":
    main()
