"""Shared loaders for the reference-produced fixtures (tests/golden/make_ref_golden.py)."""
from __future__ import annotations

import glob
import hashlib
import json
import os

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
P256_N = 0xFFFFFFFF00000000FFFFFFFFFFFFFFFFBCE6FAADA7179E84F3B9CAC2FC632551


@pytest.fixture(scope="module")
def ref():
    with open(os.path.join(HERE, "golden", "ref_golden.json")) as f:
        return json.load(f)


PART_BYTES = 900_000   # array bytes per part file: the keys are random, so a part compresses to about this


def save_parts(prefix: str, arrays: dict, limit: int = PART_BYTES) -> list:
    """Write `arrays` as prefix.00.npz, prefix.01.npz, ... of at most `limit` array bytes each
    (every committed fixture stays under 1 MiB).  A larger array is cut along axis 0 into chunks
    stored as name#0, name#1, ...; load_parts puts them together again."""
    for old in glob.glob(prefix + ".[0-9][0-9].npz"):
        os.remove(old)
    pieces = []
    for name, a in arrays.items():
        a = np.asarray(a)
        if a.nbytes <= limit:
            pieces.append((name, a))
            continue
        rows = max(1, limit // (a.nbytes // a.shape[0]))
        pieces += [(f"{name}#{k}", a[r:r + rows]) for k, r in enumerate(range(0, a.shape[0], rows))]
    parts, size = [{}], 0
    for name, a in pieces:
        if parts[-1] and size + a.nbytes > limit:
            parts.append({})
            size = 0
        parts[-1][name] = a
        size += a.nbytes
    paths = [f"{prefix}.{i:02d}.npz" for i in range(len(parts))]
    for path, part in zip(paths, parts):
        np.savez_compressed(path, **part)
    return paths


def load_parts(prefix: str) -> dict:
    """The arrays save_parts wrote under `prefix`, chunks concatenated in order."""
    paths = sorted(glob.glob(prefix + ".[0-9][0-9].npz"))
    if not paths:
        raise FileNotFoundError(prefix + ".00.npz")
    whole, chunks = {}, {}
    for path in paths:
        with np.load(path) as z:
            for key in z.files:
                if "#" in key:
                    name, k = key.split("#")
                    chunks.setdefault(name, {})[int(k)] = z[key]
                else:
                    whole[key] = z[key]
    for name, c in chunks.items():
        whole[name] = np.concatenate([c[k] for k in range(len(c))])
    return whole


@pytest.fixture(scope="module")
def refnpz():
    return load_parts(os.path.join(HERE, "golden", "ref_golden"))


def digest(v) -> str:
    return hashlib.sha256(np.ascontiguousarray(v, dtype="<u4").tobytes()).hexdigest()


def x_input(seed: int, it: int, cid: int, L: int) -> np.ndarray:
    """Same recipe as make_ref_golden.x_input (recorded in the fixture's `input` field)."""
    return np.random.Generator(np.random.PCG64([seed, it, cid])).integers(0, 2**32, size=L, dtype=np.uint32)


def key_scalar(name: str) -> int:
    """tests/golden/refshim.key_scalar: the deterministic private key per pki_files/ name."""
    return int.from_bytes(hashlib.sha512(b"refgolden-pki-" + name.encode()).digest(), "big") % (P256_N - 1) + 1


def iterations(ref):
    for run in ref["runs"]:
        for it in run["iterations"]:
            yield run, it


def client_table(run, it, npz):
    """CSR seed table of every client's y_i in the reference's own neighbour order (SA_ClientAgent.py:304-324)."""
    pre = f"{run['name']}_it{it['iteration']}_"
    m, s = npz[pre + "m"], npz[pre + "s"]
    seeds, signs, seg = [], [], [0]
    k = 0
    for c in it["clients"]:
        seeds.append(m[c["id"]])
        signs.append(1)
        for j in c["neighbors"]:
            seeds.append(s[k])
            signs.append(1 if c["id"] < j else -1)
            k += 1
        seg.append(len(seeds))
    assert k == s.shape[0]
    return np.array(seg, np.int64), np.stack(seeds), np.array(signs, np.int8)


def client_inputs(run, it):
    if run["input"].startswith("ones"):
        return None
    seed = int(run["input"].split("(")[1].split(",")[0])
    return np.stack([x_input(seed, it["iteration"], i, run["L"]) for i in range(run["N"])])


def server_table(it, npz, run):
    pre = f"{run['name']}_it{it['iteration']}_"
    sm, sp = npz[pre + "server_m"], npz[pre + "server_pairs"]
    seeds = np.concatenate([sm, sp]) if sp.size else sm
    signs = np.array([-1] * sm.shape[0] + [r[2] for r in it["recon_symbol"]], np.int8)
    return sm, sp, seeds, signs


