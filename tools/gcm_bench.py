"""Sealing and opening one BASELINE c5 iteration's m_i shares with their AES-GCM tags: 4096 clients x
the c5 committee (params.committee_size = 60) = 245,760 messages of 32 bytes, 16-byte nonces,
16-byte AAD (protocol.share_aad).

Timed in one process, on the same seeded keys, nonces and data, device-pointer forms, HIP events
around --inner back-to-back launches (one launch is tens of microseconds: the window is made long
enough to time) after --warmup untimed windows:
  seal  flm_aes_gcm_seal_dev       open  flm_aes_gcm_open_dev       xor  the unchanged flm_aes_gcm_xor_dev
The legs alternate inside every repetition.  Before anything is reported the sealed batch is opened
again (every tag verifies, the plaintext returns), its ciphertext is held to the xor leg's, and
--check rows of it to crypto.aes_gcm_seal (OpenSSL); a mismatch is an error.
  host  crypto.aes_gcm_seal row by row over the same batch on one core (--host-reps times).
--legs xor runs the xor leg alone, as does a library without the seal call (an older tree: --tree
PATH imports flamingo_amd from there): how the unchanged kernel is compared across two trees in
alternating processes, with the same launches around it in both.
One JSON line on stdout: per leg the median and min..max in ms per launch.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np


def stats(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4),
            "reps": len(ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clients", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--inner", type=int, default=50, help="launches per timed window")
    ap.add_argument("--host-reps", type=int, default=0)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--check", type=int, default=512, help="rows held to OpenSSL")
    ap.add_argument("--legs", default="xor,seal,open", help="the GPU legs to run, of xor,seal,open")
    ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.tree))
    import torch
    from flamingo_amd import MaskEngine, crypto as C, params as P

    n = a.clients * P.committee_size
    g = np.random.Generator(np.random.PCG64(245760))
    keys, nonces, aad = (g.integers(0, 256, (n, 16), dtype=np.uint8) for _ in range(3))
    data = g.integers(0, 256, (n, 32), dtype=np.uint8)
    eng = MaskEngine(0)
    asked = a.legs.split(",")
    full = hasattr(eng, "aes_gcm_seal_dev") and "seal" in asked and "open" in asked
    s = torch.cuda.Stream()
    d_k, d_n, d_a, d_d = (torch.from_numpy(x).cuda() for x in (keys, nonces, aad, data))
    new = lambda *shape: torch.zeros(shape, dtype=torch.uint8, device="cuda")  # noqa: E731
    d_ct, d_tag, d_pt, d_ok, d_x = new(n, 32), new(n, 16), new(n, 32), new(n), new(n, 32)
    legs = {"xor": lambda: eng.aes_gcm_xor_dev(d_k, d_n, d_d, out=d_x, stream=s)}
    if full:
        legs["seal"] = lambda: eng.aes_gcm_seal_dev(d_k, d_n, d_d, d_tag, out=d_ct, aad=d_a, stream=s)
        legs["open"] = lambda: eng.aes_gcm_open_dev(d_k, d_n, d_ct, d_tag, d_ok, out=d_pt, aad=d_a, stream=s)

    def window(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(s)
        for _ in range(a.inner):
            fn()
        e1.record(s)
        s.synchronize()
        return e0.elapsed_time(e1) / a.inner

    for name in ("xor", "seal", "open"):            # seal before open: open reads what seal wrote
        if name in legs:
            legs[name]()
    s.synchronize()
    kb, nb, ab, db = (x.tobytes() for x in (keys, nonces, aad, data))
    row = lambda b, w, i: b[w * i:w * i + w]  # noqa: E731
    if full:
        if not (bool((d_ok == 1).all().item()) and torch.equal(d_pt, d_d) and torch.equal(d_ct, d_x)):
            raise SystemExit("the sealed batch does not open to its plaintext, or its ciphertext is not the xor leg's")
        ct, tags = d_ct.cpu().numpy(), d_tag.cpu().numpy()
        for i in list(range(a.check // 2)) + list(range(n - a.check // 2, n)):
            want = C.aes_gcm_seal(row(kb, 16, i), row(db, 32, i), row(nb, 16, i), row(ab, 16, i))
            if (ct[i].tobytes(), tags[i].tobytes()) != want:
                raise SystemExit(f"row {i} differs from OpenSSL")
    else:
        x = d_x.cpu().numpy()
        for i in list(range(a.check // 2)) + list(range(n - a.check // 2, n)):
            if x[i].tobytes() != C.aes_gcm_encrypt(row(kb, 16, i), row(db, 32, i), row(nb, 16, i))[0]:
                raise SystemExit(f"row {i} differs from OpenSSL")
    for _ in range(a.warmup):
        for fn in legs.values():
            window(fn)
    times = {name: [] for name in legs}
    for _ in range(a.reps):
        for name, fn in legs.items():
            times[name].append(window(fn))
    out = {"tool": "gcm_bench", "messages": n, "len": 32, "nonce_len": 16, "aad_len": 16 if full else 0,
           "inner": a.inner, "checked_rows": a.check, "tree": os.path.abspath(a.tree),
           "version": eng.lib.flm_version().decode()}
    for name, ms in times.items():
        out["dev_" + name] = stats(ms)
    if full:
        out["seal_over_xor"] = round(out["dev_seal"]["median_ms"] / out["dev_xor"]["median_ms"], 3)
        out["open_over_xor"] = round(out["dev_open"]["median_ms"] / out["dev_xor"]["median_ms"], 3)
    if full and a.host_reps:
        def host():
            t0 = time.perf_counter()
            for i in range(n):
                C.aes_gcm_seal(row(kb, 16, i), row(db, 32, i), row(nb, 16, i), row(ab, 16, i))
            return (time.perf_counter() - t0) * 1e3
        out["host_seal_one_core"] = stats([host() for _ in range(a.host_reps)])
    print(json.dumps(out))
    eng.close()


if __name__ == "__main__":
    main()
