"""The DKG's Feldman share checks at the reference's default committee: n = 60 members, degree 21
(T = 22 commitments per dealer), x_bits = 6.

Timed in one process, on the same dealt polynomials (flm_shamir_deal + flm_ec_mul, as the agents deal):
  member  one member's check of SHARE_AND_COMMIT: 60 rows (every dealer's share at the member's point),
          one flm_feldman_verify host-pointer call, copies included;
  grid    the whole committee's 3,600 rows in one call (the point-major shares as they are dealt);
  dev     the same two shapes through flm_feldman_verify_dev on device-resident tensors, HIP events;
  host    the same rows through crypto.feldman_verify on one core (OpenSSL point arithmetic, the
          path of keygen.configure(gpu_dkg=False)): the member's 60 rows --host-reps times, and the
          grid's per-row cost from them.
Every verdict must be True, and the rows with one share changed False, before anything is reported.
After --warmup untimed runs each GPU leg runs --reps times; the line gives the median and the
min..max spread in ms.  One JSON line on stdout.
"""
import argparse
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


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--members", type=int, default=60)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    n = a.members
    T = int(n / 3) + 2                       # degree int(fraction n) + 1, one more coefficient
    bits = n.bit_length()
    eng = MaskEngine(0)
    g = np.random.Generator(np.random.PCG64(60))
    coeffs = g.integers(0, 256, (T, n, 32), dtype=np.uint8)
    xs = np.arange(1, n + 1, dtype=np.uint32)
    shares = eng.shamir_deal_wire(coeffs, xs)                                              # (n points, n dealers, 32)
    gw = np.tile(np.frombuffer(C.point_bytes(C.G), np.uint8), (T * n, 1))
    com = eng.ec_mul_wire(gw, coeffs.reshape(T * n, 32))[0].reshape(T, n, 64)
    grid_xs = np.repeat(xs, n)
    grid_sh = np.ascontiguousarray(shares.reshape(n * n, 32))
    member = n // 2                                                                        # the member that is timed
    mem_xs = np.full(n, member, np.uint32)
    mem_sh = np.ascontiguousarray(shares[member - 1])

    ok, fl, _ = eng.feldman_verify_wire(com, None, grid_xs, grid_sh, x_bits=bits)
    if not ok.all() or fl.any():
        raise SystemExit("an honest row failed its check")
    bad = grid_sh.copy()
    bad[:, 31] ^= 1
    if eng.feldman_verify_wire(com, None, grid_xs, bad, x_bits=bits)[0].any():
        raise SystemExit("a changed share passed its check")

    pts = [[p for p in C.points_from_wire(com[k])] for k in range(T)]
    by_dealer = [[pts[k][d] for k in range(T)] for d in range(n)]
    mem_ints = [int.from_bytes(bytes(r), "big") for r in mem_sh]

    def host_member():
        return [C.feldman_verify(mem_ints[d], member, by_dealer[d]) for d in range(n)]

    def wall(fn):
        t0 = time.perf_counter()
        r = fn()
        return r, (time.perf_counter() - t0) * 1e3

    if not all(host_member()):
        raise SystemExit("the host path refused an honest row")

    s = torch.cuda.Stream()
    d_com = torch.from_numpy(com).cuda()
    dev_in = {}
    for name, x, sh in (("member", mem_xs, mem_sh), ("grid", grid_xs, grid_sh)):
        dev_in[name] = (torch.from_numpy(x.view(np.int32)).cuda(), torch.from_numpy(sh).cuda(),
                        torch.zeros(len(x), dtype=torch.uint8, device="cuda"))

    def dev(name):
        dx, dsh, dok = dev_in[name]
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(s)
        eng.feldman_verify_dev(d_com, None, dx, dsh, bits, dok, stream=s)
        e1.record(s)
        s.synchronize()
        return e0.elapsed_time(e1)

    gpu_member = lambda: eng.feldman_verify_wire(com, None, mem_xs, mem_sh, x_bits=bits)  # noqa: E731
    gpu_grid = lambda: eng.feldman_verify_wire(com, None, grid_xs, grid_sh, x_bits=bits)  # noqa: E731
    for _ in range(a.warmup):
        gpu_member(), gpu_grid(), dev("member"), dev("grid")
    if not all(bool(dev_in[k][2].all().item()) for k in dev_in):
        raise SystemExit("the device form refused an honest row")
    t_host = [wall(host_member)[1] for _ in range(a.host_reps)]
    t_mem = [wall(gpu_member)[1] for _ in range(a.reps)]
    t_grid = [wall(gpu_grid)[1] for _ in range(a.reps)]
    t_dmem = [dev("member") for _ in range(a.reps)]
    t_dgrid = [dev("grid") for _ in range(a.reps)]
    h = statistics.median(t_host)
    print(json.dumps({
        "tool": "dkg_bench", "members": n, "commitments": T, "x_bits": bits, "all_verdicts_right": True,
        "host_one_core_member_rows": stats(t_host), "host_one_core_grid_ms_from_rows": round(h * n, 2),
        "gpu_member_host_pointer_call": stats(t_mem), "gpu_grid_host_pointer_call": stats(t_grid),
        "dev_member": stats(t_dmem), "dev_grid": stats(t_dgrid),
        "member_host_over_gpu": round(h / statistics.median(t_mem), 2),
        "grid_host_over_gpu": round(h * n / statistics.median(t_grid), 2),
        "version": eng.lib.flm_version().decode()}))
    eng.close()


if __name__ == "__main__":
    main()
