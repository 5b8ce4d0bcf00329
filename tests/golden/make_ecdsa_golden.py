"""Golden cases for the GPU ECDSA verification (flm_ecdsa_verify, ecdsa_verify_kernel).

Every case is built on the CPU from the affine arithmetic of oracle/ec_oracle.py: signatures are
made in plain Python with nonces derived from the case's label (so the file is reproducible), and
the expected verdict and flags come from `verify` below, FIPS 186-4 section 6.4.2 in plain Python.
The generator then asserts that OpenSSL's digest-level ECDSA_do_verify
(flamingo_amd.crypto.ecdsa_verify_digest) gives the same verdict for every case.
``python tests/golden/make_ecdsa_golden.py`` rewrites ecdsa_golden.json; tests/test_ecdsa_cpu.py
re-runs it in memory.

A case: {"name", "q" (64 wire bytes), "e" (32-byte digest), "r", "s" (32 bytes each), all hex,
"ok" (bool), "flags"}; flags bit 0: r or s outside [1, n-1], bit 1: q not a valid point, bit 2:
u1 G + u2 Q at infinity.
"""
from __future__ import annotations

import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, "ecdsa_golden.json")
for _p in (ROOT, os.path.join(ROOT, "oracle")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import ec_oracle as E  # noqa: E402

P, N, G = E.P, E.N, E.G
TOP = (1 << 256) - 1


def h_int(label: str) -> int:
    return int.from_bytes(hashlib.sha256(label.encode()).digest(), "big")


def b32(v: int) -> bytes:
    return int(v).to_bytes(32, "big")


def verify(q: bytes, e: bytes, r: int, s: int):
    """(verdict, flags) of one row, every check evaluated as the kernel reports it."""
    flags = 0
    if not (1 <= r < N and 1 <= s < N):
        flags |= 1
    x, y = int.from_bytes(q[:32], "big"), int.from_bytes(q[32:], "big")
    if x >= P or y >= P or not E.on_curve((x, y)) or q == bytes(64):
        flags |= 2
    if flags:
        return False, flags
    w = pow(s, -1, N)
    u1, u2 = int.from_bytes(e, "big") % N * w % N, r * w % N
    R = E.add(E.mul(u1), E.mul(u2, (x, y)))
    if R is None:
        return False, 4
    return R[0] % N == r, 0


def sign(d: int, e: bytes, label: str):
    """(r, s) over the digest e with the nonce derived from the label"""
    ctr = 0
    while True:
        k = h_int(f"nonce:{label}:{ctr}") % (N - 1) + 1
        r = E.mul(k)[0] % N
        s = pow(k, -1, N) * (int.from_bytes(e, "big") + r * d) % N
        if r and s:
            return r, s
        ctr += 1


def case(name: str, q: bytes, e: bytes, r: int, s: int) -> dict:
    ok, flags = verify(q, e, r, s)
    return {"name": name, "q": q.hex(), "e": e.hex(), "r": b32(r).hex(), "s": b32(s).hex(), "ok": ok, "flags": flags}


def flip(b: bytes, bit: int) -> bytes:
    out = bytearray(b)
    out[bit >> 3] ^= 1 << (bit & 7)
    return bytes(out)


def signed_with_twins(name: str, d: int, e: bytes) -> list:
    """a genuine signature under d and its four tampered twins (one bit of r, s, e, Q)"""
    q = E.wire(E.mul(d))
    r, s = sign(d, e, name)
    bit = h_int(f"bit:{name}")
    out = [case(name, q, e, r, s),
           case(name + "/r-bit", q, e, r ^ (1 << (bit % 256)), s),
           case(name + "/s-bit", q, e, r, s ^ (1 << ((bit >> 8) % 256))),
           case(name + "/e-bit", q, flip(e, (bit >> 16) % 256), r, s),
           case(name + "/q-bit", flip(q, (bit >> 24) % 512), e, r, s)]
    assert out[0]["ok"], name
    return out


def sqrt_p(v: int):
    y = pow(v, (P + 1) // 4, P)
    return y if y * y % P == v % P else None


def build() -> list:
    cases = []
    # random valid signatures, each with one bit flipped in r, s, the digest and Q
    for i in range(8):
        d = h_int(f"key:{i}") % (N - 1) + 1
        cases += signed_with_twins(f"random{i}", d, hashlib.sha256(f"message {i}".encode()).digest())
    assert any(c["flags"] == 2 for c in cases)      # a flipped Q leaves the curve
    # high s: (r, n - s) verifies with (r, s)
    d = h_int("key:high-s") % (N - 1) + 1
    q, e = E.wire(E.mul(d)), hashlib.sha256(b"high s").digest()
    r, s = sign(d, e, "high-s")
    cases += [case("low-or-high-s", q, e, r, s), case("the-other-s", q, e, r, N - s)]
    # digests 0^32 and 0xFF^32 (>= n), signed accordingly, and crossed
    d = h_int("key:digests") % (N - 1) + 1
    q = E.wire(E.mul(d))
    for nm, e in (("digest-zero", bytes(32)), ("digest-ff", b"\xff" * 32)):
        r, s = sign(d, e, nm)
        cases.append(case(nm, q, e, r, s))
        cases.append(case(nm + "/other-digest", q, bytes(32) if e[0] else b"\xff" * 32, r, s))
    # e and e + n are the same digest mod n
    e_small = b32(h_int("digest:small") % (TOP - N))
    r, s = sign(d, e_small, "digest-plus-n")
    cases += [case("digest-small", q, e_small, r, s),
              case("digest-plus-n", q, b32(int.from_bytes(e_small, "big") + N), r, s)]
    # r or s out of range
    e = hashlib.sha256(b"range").digest()
    r, s = sign(d, e, "range")
    for nm, rr, ss in (("r-zero", 0, s), ("s-zero", r, 0), ("r-is-n", N, s), ("s-is-n", r, N), ("r-top", TOP, s),
                       ("s-top", r, TOP), ("r-plus-n", r + N if r + N <= TOP else N + 1, s), ("both-zero", 0, 0)):
        cases.append(case(nm, q, e, rr, ss))
    # invalid keys: infinity's wire form, coordinates >= p (x = p is 0 mod p, and (0, sqrt b) is a point)
    yb = sqrt_p(E.B)
    assert yb is not None and E.on_curve((0, yb))
    x1 = next(x for x in range(1, 1000) if sqrt_p(x ** 3 + E.A * x + E.B) is not None)
    cases += [case("q-zero-bytes", bytes(64), e, r, s),
              case("q-x-is-p", b32(P) + b32(yb), e, r, s),
              case("q-x-zero-on-curve", b32(0) + b32(yb), e, r, s),       # valid key, wrong signature
              case("q-y-is-p-plus", b32(x1) + b32(TOP), e, r, s),
              case("q-x-top", b32(TOP) + q[32:], e, r, s),
              case("q-y-negated", q[:32] + b32(P - int.from_bytes(q[32:], "big")), e, r, s),
              case("q-zero-and-r-zero", bytes(64), e, 0, s)]
    # x(R) >= n: R the first curve point with x > n, r = x - n
    x = N + 1
    while sqrt_p(x ** 3 + E.A * x + E.B) is None:
        x += 1
    assert x < P
    R = (x, sqrt_p(x ** 3 + E.A * x + E.B))
    r, s, e = x - N, h_int("xr:s") % (N - 1) + 1, hashlib.sha256(b"x(R) >= n").digest()
    w = pow(s, -1, N)
    u1, u2 = int.from_bytes(e, "big") % N * w % N, r * w % N
    q_x = E.wire(E.mul(pow(u2, -1, N), E.add(R, E.neg(E.mul(u1)))))
    cases += [case("xR-above-n", q_x, e, r, s), case("xR-above-n/r-is-x", q_x, e, x % (1 << 256), s),
              case("xR-above-n/s-bit", q_x, e, r, s ^ 2)]
    assert cases[-3]["ok"]
    # u1 G + u2 Q at infinity: e = -r d mod n
    d = h_int("key:infinity") % (N - 1) + 1
    r, s = h_int("inf:r") % (N - 1) + 1, h_int("inf:s") % (N - 1) + 1
    cases.append(case("sum-at-infinity", E.wire(E.mul(d)), b32(-r * d % N), r, s))
    assert cases[-1]["flags"] == 4
    # u1 G = u2 Q (the last addition is a doubling): R = 2t G, r = x(R) mod n, s = r d / t, e = t s
    t = h_int("dbl:t") % (N - 1) + 1
    r = E.mul(2 * t % N)[0] % N
    s = r * d * pow(t, -1, N) % N
    cases += [case("u1G-equals-u2Q", E.wire(E.mul(d)), b32(t * s % N), r, s),
              case("u1G-equals-u2Q/r-bit", E.wire(E.mul(d)), b32(t * s % N), r ^ 1, s)]
    assert cases[-2]["ok"]
    # keys whose tables of odd multiples collide with G's
    for d in (1, 2, 3, N - 1, N - 2):
        nm = f"key-{d}" if d < 4 else f"key-n-minus-{N - d}"
        cases += signed_with_twins(nm, d, hashlib.sha256(nm.encode()).digest())
    names = [c["name"] for c in cases]
    assert len(set(names)) == len(names)
    return cases


def check_against_openssl(cases) -> int:
    """OpenSSL's ECDSA_do_verify on the digest agrees with every plain-Python verdict."""
    from flamingo_amd import crypto as C
    for c in cases:
        q = bytes.fromhex(c["q"])
        pub = (int.from_bytes(q[:32], "big"), int.from_bytes(q[32:], "big"))
        got = C.ecdsa_verify_digest(None if q == bytes(64) else pub, bytes.fromhex(c["e"]),
                                    bytes.fromhex(c["r"]) + bytes.fromhex(c["s"]))
        assert got == c["ok"], (c["name"], got, c["ok"])
    return len(cases)


def load() -> list:
    with open(OUT) as f:
        return json.load(f)["cases"]


def main():
    cases = build()
    n = check_against_openssl(cases)
    with open(OUT, "w") as f:
        json.dump({"cases": cases}, f, indent=0)
        f.write("\n")
    print(f"{OUT}: {n} cases ({sum(c['ok'] for c in cases)} valid), {os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    main()
