"""Record flm_plan_aggregate's output per shape into tests/golden/planner_items.json: the SHA-256 of
the returned item bytes (order included), n_items and plan_flags.  tests/test_planner_cpu.py
recomputes and compares, so a change of the planner that moves, reorders or re-flags an item shows.

    python tools/record_planner_items.py          # needs the built library, no GPU

Run it on the commit whose plans are the reference, never to make a failing comparison pass."""
from __future__ import annotations

import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
OUT = os.path.join(ROOT, "tests", "golden", "planner_items.json")
FIELDS = ("subtiles", "pairing", "N", "K", "L", "lo", "hi", "prg_slot0")


def shapes():
    """The pinned shapes as dicts of FIELDS (the pitch is always round_up(L, 64))."""
    import test_planner_cpu as T
    out = []

    def add(N, K, L, lo=0, hi=None, pairing=1, subtiles=0, prg_slot0=0):
        s = dict(subtiles=subtiles, pairing=pairing, N=N, K=K, L=L, lo=lo, hi=L if hi is None else hi,
                 prg_slot0=prg_slot0)
        if s not in out:
            out.append(s)

    for N, K, L, lo, hi, pairing in T.COVER_SHAPES:
        add(N, K, L, lo, hi, pairing)
    for N, K, L, lo, hi, pairing in T.MODE_SHAPES:
        add(N, K, L, lo, hi, pairing)
    for shape in ((1024, 8192, 1 << 20, 3 << 17, 4 << 17), (128, 156, 16000, 0, 16000)):
        for subtiles in (0, 1, 4, 16):
            for pairing in (0, 1, 2):
                add(*shape, pairing=pairing, subtiles=subtiles)
    for slot0 in (0, 16, (1 << 36) - 16000):
        add(128, 156, 16000, 0, 16000, prg_slot0=slot0)
    return out


def digest(s):
    """(n_items, plan_flags, sha256 of the item bytes) of one shape, through the library."""
    import test_planner_cpu as T
    items, flags, _ = T.plan(s["N"], s["K"], s["L"], s["lo"], s["hi"], prg_slot0=s["prg_slot0"],
                             subtiles=s["subtiles"], pairing=s["pairing"])
    assert items.dtype.itemsize == 64
    return len(items), flags, hashlib.sha256(items.tobytes()).hexdigest()


def main():
    rec = []
    for s in shapes():
        n, flags, sha = digest(s)
        rec.append(dict(s, n_items=n, plan_flags=flags, sha256=sha))
    with open(OUT, "w") as f:
        f.write("[\n" + ",\n".join(" " + json.dumps(r) for r in rec) + "\n]\n")
    print(f"{len(rec)} shapes -> {os.path.relpath(OUT, ROOT)}")


if __name__ == "__main__":
    main()
