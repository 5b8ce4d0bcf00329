"""Golden cases for the GPU dealing and sealing of the m_i shares (flm_shamir_deal, flm_aes_gcm_xor).

Generated on the CPU with the product's own host restatements: the Shamir cases by
seeds.shamir_share's arithmetic (Python Horner mod n), the AES cases by crypto.aes_gcm_encrypt
(OpenSSL, tag dropped).  ``python tests/golden/make_deal_golden.py`` rewrites deal_golden.json;
tests/test_deal_cpu.py re-runs it in memory.

AES cases: every length of AES_LENS at n = 1 and 65; batches around one and two 256-message
workgroups (AES_BATCH_NS); and the counter-wrap cases (aes_wrap_case), whose first rows carry
16-byte nonces solved in GF(2^128) so that J0's low word is at the top of its range and inc32 wraps
inside the message.  Their expected bytes are OpenSSL's like all the others.

A byte field of the JSON has one of three forms, so that the file stays small:
  base64 text                               the bytes (edge inputs, expected outputs up to 1 KiB);
  {"prg", "n", "set": [[offset, b64]...]}   seeded random inputs: SHA-256 in counter mode over the
                                            label, the listed edge values written over it;
  {"sha256", "n"}                           a longer expected output, pinned by its digest: a test
                                            recomputes it (shamir_expected / aes_expected), checks
                                            the digest (field_matches) and compares against that.
"""
from __future__ import annotations

import base64
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "deal_golden.json")
N = 0xFFFFFFFF00000000FFFFFFFFFFFFFFFFBCE6FAADA7179E84F3B9CAC2FC632551     # seeds.P256_N
X_MAX, TOP = (1 << 32) - 1, (1 << 256) - 1
AES_LENS = (1, 15, 16, 17, 32, 33, 64, 256)


def prg(label: str, n: int) -> bytes:
    return b"".join(hashlib.sha256(f"{label}:{c}".encode()).digest() for c in range((n + 31) // 32))[:n]


def _b64(b: bytes) -> str:
    return base64.b64encode(b).decode()


def prg_field(label: str, n: int, patches=()) -> dict:
    return {"prg": label, "n": n, "set": [[int(o), _b64(b)] for o, b in patches]}


def out_field(b: bytes):
    return _b64(b) if len(b) <= 1024 else {"sha256": hashlib.sha256(b).hexdigest(), "n": len(b)}


def field_bytes(f) -> bytes:
    if isinstance(f, str):
        return base64.b64decode(f)
    b = bytearray(prg(f["prg"], f["n"]))
    for off, patch in f["set"]:
        p = base64.b64decode(patch)
        b[off:off + len(p)] = p
    return bytes(b)


def field_matches(f, b: bytes) -> bool:
    if isinstance(f, dict) and "sha256" in f:
        return len(b) == f["n"] and hashlib.sha256(b).hexdigest() == f["sha256"]
    return field_bytes(f) == b


# (T, C, M) -> (xs, [(flat coefficient index j * M + i, edge value)]); the rest is seeded random,
# any 32 bytes (m_i may exceed n)
SHAMIR = {
    (1, 1, 1): ([1], [(0, N + 1)]),
    (1, 3, 2): ([2, 2, X_MAX], [(0, N), (1, TOP)]),
    (2, 3, 1): ([1, 2, X_MAX], [(0, N - 1), (1, 0)]),
    (3, 5, 65): ([1, 2, 2, X_MAX, 7], [(0, 0), (1, 1), (64, N - 1), (65, N), (130, N + 1), (194, TOP)]),
    (40, 60, 130): (list(range(1, 61)), [(0, TOP), (129, N), (130, 0), (2600, 1), (39 * 130, N - 1), (5199, N + 1)]),
}


def shamir_expected(case: dict) -> bytes:
    """C x M x 32 bytes: f_i(x_c) mod n from the top coefficient down, as seeds.shamir_share."""
    T, M, raw = case["T"], case["M"], field_bytes(case["coeffs"])
    co = [int.from_bytes(raw[32 * k:32 * k + 32], "big") % N for k in range(T * M)]
    out = []
    for x in case["xs"]:
        for i in range(M):
            y = 0
            for j in reversed(range(T)):
                y = (y * x + co[j * M + i]) % N
            out.append(y.to_bytes(32, "big"))
    return b"".join(out)


def aes_expected(case: dict) -> bytes:
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    from flamingo_amd import crypto as C
    nl, ln, n = case["nonce_len"], case["len"], case["n"]
    k, nc, d = (field_bytes(case[f]) for f in ("keys", "nonces", "data"))
    return b"".join(C.aes_gcm_encrypt(k[16 * i:16 * i + 16], d[ln * i:ln * i + ln], nc[nl * i:nl * i + nl])[0]
                    for i in range(n))


_expected: dict = {}


def expected(case: dict) -> bytes:
    """A loaded case's expected output: recomputed on the CPU once, held to the committed field."""
    if case["name"] not in _expected:
        b = shamir_expected(case) if "shares" in case else aes_expected(case)
        assert field_matches(case["shares"] if "shares" in case else case["out"], b), case["name"]
        _expected[case["name"]] = b
    return _expected[case["name"]]


def shamir_case(T: int, C: int, M: int) -> dict:
    xs, edges = SHAMIR[(T, C, M)]
    case = {"name": f"shamir_T{T}_C{C}_M{M}", "T": T, "C": C, "M": M, "xs": xs,
            "coeffs": prg_field(f"shamir-{T}-{C}-{M}", T * M * 32, [(32 * k, v.to_bytes(32, "big")) for k, v in edges])}
    case["shares"] = out_field(shamir_expected(case))
    return case


def aes_case(nl: int, ln: int, n: int, kind: int) -> dict:
    """Message 0: all-zero key and nonce; 1: all 0xFF; 2: zero key, 0xFF nonce; the rest seeded
    random.  n = 1: `kind` 0 / 1 / 2 picks the first, the second or a random one."""
    fixed = [(b"\x00", b"\x00"), (b"\xff", b"\xff"), (b"\x00", b"\xff")]
    which = [(0, kind)] if n == 1 else [(i, i) for i in range(3)]
    which = [(i, k) for i, k in which if n > 1 or k < 2]
    label = f"aes-{nl}-{ln}-{n}-{kind}"
    case = {"name": f"aes_nonce{nl}_len{ln}_n{n}", "nonce_len": nl, "len": ln, "n": n,
            "keys": prg_field(label + "-k", 16 * n, [(16 * i, fixed[k][0] * 16) for i, k in which]),
            "nonces": prg_field(label + "-n", nl * n, [(nl * i, fixed[k][1] * nl) for i, k in which]),
            "data": prg_field(label + "-d", ln * n)}
    case["out"] = out_field(aes_expected(case))
    return case


# ---- counter wrap: 16-byte nonces solved for a chosen J0 (NIST SP 800-38D, 7.1: keystream block m is
# E_k(inc32^m(J0)), and inc32 wraps the low 32 bits without a carry into the upper 96)
GCM_R = 0xE1 << 120
AES_BATCH_NS = (255, 256, 257, 513)            # around one and two workgroups of the kernel (256 messages each)
WRAP_LENS, WRAP_N = (17, 32, 256), 65
WRAP_HIGH = 0x0123456789ABCDEFFFFFFFFF          # J0's upper 96 bits: a 64- or 128-bit increment would carry into them
WRAP_LOWS = (0xFFFFFFFF, 0xFFFFFFFE, 0xFFFFFFF0)


def gf_mul(x: int, y: int) -> int:
    """x * y in GF(2^128) as GCM orders its bits (bit 0 = the top bit of byte 0)."""
    z = 0
    for i in range(127, -1, -1):
        if (x >> i) & 1:
            z ^= y
        y = (y >> 1) ^ (GCM_R if y & 1 else 0)
    return z


def gf_inv(x: int) -> int:
    """x^(2^128 - 2): square and multiply from the one, 1 || 0^127."""
    r, e = 1 << 127, (1 << 128) - 2
    while e:
        if e & 1:
            r = gf_mul(r, x)
        x, e = gf_mul(x, x), e >> 1
    return r


def aes_ecb_block(key16: bytes, block16: bytes) -> bytes:
    """E_k(block) through OpenSSL's EVP_aes_128_ecb (bound here: the product never needs it)."""
    import ctypes
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    from flamingo_amd import crypto as C
    c = C._lib()
    c.EVP_aes_128_ecb.restype, c.EVP_aes_128_ecb.argtypes = ctypes.c_void_p, []
    ctx = c.EVP_CIPHER_CTX_new()
    try:
        assert c.EVP_EncryptInit_ex(ctx, c.EVP_aes_128_ecb(), None, key16, None) == 1
        out, n = ctypes.create_string_buffer(32), ctypes.c_int(0)
        assert c.EVP_EncryptUpdate(ctx, out, ctypes.byref(n), block16, 16) == 1 and n.value == 16
        return out.raw[:16]
    finally:
        c.EVP_CIPHER_CTX_free(ctx)


def gcm_j0(key16: bytes, nonce16: bytes) -> int:
    """J0 = GHASH_H(nonce || 0^64 || [128]_64) of a 16-byte nonce, H = E_k(0^128)."""
    h = int.from_bytes(aes_ecb_block(key16, bytes(16)), "big")
    return gf_mul(gf_mul(int.from_bytes(nonce16, "big"), h) ^ 128, h)


def nonce_for_j0(key16: bytes, j0: int) -> bytes:
    """The 16-byte nonce whose J0 is j0: ((j0 H^-1) ^ [128]) H^-1."""
    hi = gf_inv(int.from_bytes(aes_ecb_block(key16, bytes(16)), "big"))
    return gf_mul(gf_mul(j0, hi) ^ 128, hi).to_bytes(16, "big")


def wrap_lows(ln: int) -> tuple:
    """The low words of J0 of a wrap case's crafted rows, three rows (keys) each: WRAP_LOWS, then the
    last one that still wraps for this length -- the counter of the final block is 0."""
    return WRAP_LOWS + ((1 << 32) - (ln + 15) // 16,)


def aes_wrap_case(ln: int) -> dict:
    """nonce_len 16, n = 65.  Row 3 q + kind has J0 = WRAP_HIGH || wrap_lows(ln)[q] under the all-zero
    key (kind 0), the all-0xFF key (1) or the row's own seeded key (2); the other rows are seeded."""
    label, n, lows = f"aes-wrap-{ln}", WRAP_N, wrap_lows(ln)
    rows = 3 * len(lows)
    keys = bytearray(prg(label + "-k", 16 * n))
    kp, np_ = [], []
    for i in range(rows):
        if i % 3 < 2:
            kp.append((16 * i, (b"\x00", b"\xff")[i % 3] * 16))
            keys[16 * i:16 * i + 16] = kp[-1][1]
        np_.append((16 * i, nonce_for_j0(bytes(keys[16 * i:16 * i + 16]), (WRAP_HIGH << 32) | lows[i // 3])))
    case = {"name": f"aes_wrap_len{ln}_n{n}", "nonce_len": 16, "len": ln, "n": n, "wrap_rows": rows,
            "keys": prg_field(label + "-k", 16 * n, kp), "nonces": prg_field(label + "-n", 16 * n, np_),
            "data": prg_field(label + "-d", ln * n)}
    case["out"] = out_field(aes_expected(case))
    return case


def generate() -> dict:
    aes = [aes_case(nl, ln, n, q % 3) for nl in (12, 16) for q, ln in enumerate(AES_LENS) for n in (1, 65)]
    aes += [aes_case(nl, 32, n, 0) for nl in (12, 16) for n in AES_BATCH_NS]
    aes += [aes_wrap_case(ln) for ln in WRAP_LENS]
    return {"n": hex(N), "shamir": [shamir_case(*k) for k in SHAMIR], "aes": aes}


def load() -> dict:
    with open(OUT) as f:
        return json.load(f)


if __name__ == "__main__":
    g = generate()
    rows = lambda cases: ",\n".join(json.dumps(c, sort_keys=True) for c in cases)  # noqa: E731
    with open(OUT, "w") as f:               # one case per line
        f.write('{"n": "%s",\n"shamir": [\n%s],\n"aes": [\n%s]}\n' % (g["n"], rows(g["shamir"]), rows(g["aes"])))
    print(OUT, os.path.getsize(OUT), "bytes")
