"""Golden cases for AES-128-GCM with its tag on the GPU (flm_aes_gcm_seal, flm_aes_gcm_open).

Expected ciphertexts and tags come from OpenSSL through crypto.aes_gcm_seal.  ``python
tests/golden/make_gcm_golden.py`` rewrites gcm_golden.json; tests/test_gcm_cpu.py re-runs it in
memory.  The byte fields have make_deal_golden.py's compact forms (its helpers are imported, not
restated), and so do the fixed first rows: message 0 all-zero key and nonce, 1 all 0xFF, 2 zero key
with 0xFF nonce.

Cases:
  every len of LENS x aad_len of AADS x nonce_len 12 and 16, at n = 65;
  the AAD lengths around one and two GHASH blocks and the longest (AADS_ONE), at len 32, n = 1;
  batches around one and two 256-message workgroups (BATCH_NS), len 32, aad_len 16, nonce_len 16;
  the counter-wrap rows (wrap_case): 16-byte nonces solved for a J0 whose low word is 0xFFFFFFFF or
  0xFFFFFFFE, so the keystream counter wraps inside the message while the tag is masked with the
  un-incremented J0;
  the four AES-128 test cases of the GCM specification (McGrew & Viega, appendix B), as literals.
"""
from __future__ import annotations

import importlib.util
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "gcm_golden.json")


def _deal():
    spec = importlib.util.spec_from_file_location("make_deal_golden", os.path.join(HERE, "make_deal_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


D = _deal()
LENS = (0, 1, 15, 16, 17, 32, 33, 256)
AADS = (0, 16, 20)
AADS_ONE = (1, 15, 17, 64)
BATCH_NS = (255, 256, 257, 513)
WRAP_LENS, WRAP_N, WRAP_LOWS = (17, 32), 65, (0xFFFFFFFF, 0xFFFFFFFE)

# key, iv, plaintext, aad, ciphertext, tag
SPEC_VECTORS = (
    ("00000000000000000000000000000000", "000000000000000000000000", "", "", "",
     "58e2fccefa7e3061367f1d57a4e7455a"),
    ("00000000000000000000000000000000", "000000000000000000000000", "00000000000000000000000000000000", "",
     "0388dace60b6a392f328c2b971b2fe78", "ab6e47d42cec13bdf53a67b21257bddf"),
    ("feffe9928665731c6d6a8f9467308308", "cafebabefacedbaddecaf888",
     "d9313225f88406e5a55909c5aff5269a86a7a9531534f7da2e4c303d8a318a721c3c0c95956809532fcf0e2449a6b525"
     "b16aedf5aa0de657ba637b391aafd255", "",
     "42831ec2217774244b7221b784d0d49ce3aa212f2c02a4e035c17e2329aca12e21d514b25466931c7d8f6a5aac84aa05"
     "1ba30b396a0aac973d58e091473f5985", "4d5c2af327cd64a62cf35abd2ba6fab4"),
    ("feffe9928665731c6d6a8f9467308308", "cafebabefacedbaddecaf888",
     "d9313225f88406e5a55909c5aff5269a86a7a9531534f7da2e4c303d8a318a721c3c0c95956809532fcf0e2449a6b525"
     "b16aedf5aa0de657ba637b39", "feedfacedeadbeeffeedfacedeadbeefabaddad2",
     "42831ec2217774244b7221b784d0d49ce3aa212f2c02a4e035c17e2329aca12e21d514b25466931c7d8f6a5aac84aa05"
     "1ba30b396a0aac973d58e091", "5bc94fbc3221a5db94fae95ae7121a47"),
)


def _crypto():
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    from flamingo_amd import crypto as C
    return C


def gcm_expected(case: dict) -> tuple:
    """(ciphertexts n x len, tags n x 16) of a case, row by row through OpenSSL."""
    C = _crypto()
    nl, al, ln, n = case["nonce_len"], case["aad_len"], case["len"], case["n"]
    k, nc, a, d = (D.field_bytes(case[f]) for f in ("keys", "nonces", "aad", "data"))
    rows = [C.aes_gcm_seal(k[16 * i:16 * i + 16], d[ln * i:ln * i + ln], nc[nl * i:nl * i + nl], a[al * i:al * i + al])
            for i in range(n)]
    return b"".join(r[0] for r in rows), b"".join(r[1] for r in rows)


_expected: dict = {}


def expected(case: dict) -> tuple:
    """A loaded case's expected (ciphertexts, tags): recomputed once, held to the committed fields."""
    if case["name"] not in _expected:
        ct, tags = gcm_expected(case)
        assert D.field_matches(case["ct"], ct) and D.field_matches(case["tags"], tags), case["name"]
        _expected[case["name"]] = (ct, tags)
    return _expected[case["name"]]


def _finish(case: dict) -> dict:
    ct, tags = gcm_expected(case)
    case["ct"], case["tags"] = D.out_field(ct), D.out_field(tags)
    return case


def gcm_case(nl: int, al: int, ln: int, n: int) -> dict:
    fixed = [(b"\x00", b"\x00"), (b"\xff", b"\xff"), (b"\x00", b"\xff")] if n > 1 else []
    label = f"gcm-{nl}-{al}-{ln}-{n}"
    return _finish({"name": f"gcm_nonce{nl}_aad{al}_len{ln}_n{n}", "nonce_len": nl, "aad_len": al, "len": ln, "n": n,
                    "keys": D.prg_field(label + "-k", 16 * n, [(16 * i, f[0] * 16) for i, f in enumerate(fixed)]),
                    "nonces": D.prg_field(label + "-n", nl * n, [(nl * i, f[1] * nl) for i, f in enumerate(fixed)]),
                    "aad": D.prg_field(label + "-a", al * n), "data": D.prg_field(label + "-d", ln * n)})


def wrap_case(ln: int) -> dict:
    """nonce_len 16, aad_len 16, n = 65.  Row 3 q + kind has J0 = WRAP_HIGH || WRAP_LOWS[q] under the
    all-zero key (kind 0), the all-0xFF key (1) or the row's own seeded key (2)."""
    label, n = f"gcm-wrap-{ln}", WRAP_N
    rows = 3 * len(WRAP_LOWS)
    keys = bytearray(D.prg(label + "-k", 16 * n))
    kp, np_ = [], []
    for i in range(rows):
        if i % 3 < 2:
            kp.append((16 * i, (b"\x00", b"\xff")[i % 3] * 16))
            keys[16 * i:16 * i + 16] = kp[-1][1]
        np_.append((16 * i, D.nonce_for_j0(bytes(keys[16 * i:16 * i + 16]), (D.WRAP_HIGH << 32) | WRAP_LOWS[i // 3])))
    return _finish({"name": f"gcm_wrap_len{ln}_n{n}", "nonce_len": 16, "aad_len": 16, "len": ln, "n": n, "wrap_rows": rows,
                    "keys": D.prg_field(label + "-k", 16 * n, kp), "nonces": D.prg_field(label + "-n", 16 * n, np_),
                    "aad": D.prg_field(label + "-a", 16 * n), "data": D.prg_field(label + "-d", ln * n)})


def spec_case(t: int, vec: tuple) -> dict:
    """A test case of the specification: the literal fields, not recomputed here: expected() holds OpenSSL to them."""
    key, iv, pt, aad, ct, tag = (bytes.fromhex(v) for v in vec)
    return {"name": f"gcm_spec_tc{t}", "nonce_len": len(iv), "aad_len": len(aad), "len": len(pt), "n": 1,
            "keys": D._b64(key), "nonces": D._b64(iv), "aad": D._b64(aad), "data": D._b64(pt),
            "ct": D._b64(ct), "tags": D._b64(tag)}


def generate() -> dict:
    cases = [gcm_case(nl, al, ln, 65) for nl in (12, 16) for al in AADS for ln in LENS]
    cases += [gcm_case(16, al, 32, 1) for al in AADS_ONE]
    cases += [gcm_case(16, 16, 32, n) for n in BATCH_NS]
    cases += [wrap_case(ln) for ln in WRAP_LENS]
    cases += [spec_case(t + 1, v) for t, v in enumerate(SPEC_VECTORS)]
    return {"gcm": cases}


def load() -> dict:
    with open(OUT) as f:
        return json.load(f)


if __name__ == "__main__":
    g = generate()
    with open(OUT, "w") as f:               # one case per line
        f.write('{"gcm": [\n%s]}\n' % ",\n".join(json.dumps(c, sort_keys=True) for c in g["gcm"]))
    print(OUT, os.path.getsize(OUT), "bytes")
