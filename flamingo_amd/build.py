"""Build libflamingo_hip.so in-tree for gfx950 (hipcc, no JIT cache), and beside it the test-only
libflm_fieldtest.so (tests/fieldtest/flm_fieldtest.hip: the field layers one operation per kernel,
for tests/test_fe_ops_gpu.py; never linked into the product library).

``python -m flamingo_amd.build`` or ``flamingo_amd.build.build()``.  The .so
files land in flamingo_amd/lib/ (git-ignored, shipped to the GPU box with the tree).
"""
from __future__ import annotations

import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = [os.path.join(HERE, "csrc", f) for f in ("flm_kernels.hip", "flm_runtime.hip", "flm_p256.hip", "flm_comm.hip",
                                                        "flm_store.hip")]
# every header makes the library stale: no list to keep by hand (tests/test_lib_abi.py checks the includes)
HDRS = sorted(os.path.join(HERE, "csrc", f) for f in os.listdir(os.path.join(HERE, "csrc")) if f.endswith(".h")) + \
    [os.path.join(os.path.dirname(HERE), "include", "flamingo_hip.h")]
OUT = os.path.join(HERE, "lib", "libflamingo_hip.so")
FIELDTEST_SRC = os.path.join(os.path.dirname(HERE), "tests", "fieldtest", "flm_fieldtest.hip")
FIELDTEST_OUT = os.path.join(HERE, "lib", "libflm_fieldtest.so")
ARCH = os.environ.get("FLM_OFFLOAD_ARCH", "gfx950")


def _newer(out: str, deps) -> bool:
    if not os.path.exists(out):
        return True
    t = os.path.getmtime(out)
    return any(os.path.getmtime(p) > t for p in deps)


def _stale() -> bool:
    return _newer(OUT, SRC + HDRS)


def _fieldtest_stale() -> bool:
    return _newer(FIELDTEST_OUT, [FIELDTEST_SRC] + HDRS)


def build(force: bool = False, verbose: bool = False) -> str:
    # each library is rebuilt when its own sources or any header is newer than it
    targets = [(OUT, SRC)] if force or _stale() else []
    if force or _fieldtest_stale():
        targets.append((FIELDTEST_OUT, [FIELDTEST_SRC]))
    if not targets:
        return OUT
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    # one hipcc per source, in parallel, then one link per library (the P-256 and kernel files dominate)
    procs, links = [], []
    for out, srcs in targets:
        objs = [os.path.join(os.path.dirname(out), os.path.basename(s) + ".o") for s in srcs]
        links.append((out, objs))
        for s, o in zip(srcs, objs):
            cmd = ["hipcc", f"--offload-arch={ARCH}", "-O3", "-std=c++17", "-fPIC", "-Wall", "-c", "-o", o, s]
            if verbose:
                print(" ".join(cmd))
            procs.append((subprocess.Popen(cmd), cmd))
    for p, cmd in procs:
        if p.wait() != 0:
            raise subprocess.CalledProcessError(p.returncode, cmd)
    for out, objs in links:
        cmd = ["hipcc", f"--offload-arch={ARCH}", "-fPIC", "-shared", "-o", out + ".tmp"] + objs
        if verbose:
            print(" ".join(cmd))
        subprocess.run(cmd, check=True)
        for o in objs:
            os.remove(o)
        os.replace(out + ".tmp", out)
    return OUT


if __name__ == "__main__":
    print(build(force="--force" in sys.argv, verbose=True))
