"""The CPU side of AES-128-GCM with its tag: the fixture regenerates to the committed file and holds the
specification's own vectors, crypto.aes_gcm_seal / aes_gcm_open (OpenSSL) against the tag-dropping
pair and against every kind of tampering, the argument rules through the stand-alone checker, and
the declarations of the four calls."""
from __future__ import annotations

import importlib.util
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _generator():
    spec = importlib.util.spec_from_file_location("make_gcm_golden",
                                                  os.path.join(ROOT, "tests", "golden", "make_gcm_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


G = _generator()
SPEC_TAGS = ("58e2fccefa7e3061367f1d57a4e7455a", "ab6e47d42cec13bdf53a67b21257bddf",
             "4d5c2af327cd64a62cf35abd2ba6fab4", "5bc94fbc3221a5db94fae95ae7121a47")


def test_fixture_regenerates():
    cases = G.generate()
    assert cases == G.load()
    assert os.path.getsize(G.OUT) < 128 * 1024
    by = {c["name"]: c for c in cases["gcm"]}
    assert len(by) == len(cases["gcm"])
    for nl in (12, 16):
        for al in (0, 16, 20):
            for ln in (0, 1, 15, 16, 17, 32, 33, 256):
                c = by[f"gcm_nonce{nl}_aad{al}_len{ln}_n65"]
                k, nc = G.D.field_bytes(c["keys"]), G.D.field_bytes(c["nonces"])
                assert k[:48] == bytes(16) + b"\xff" * 16 + bytes(16)
                assert nc[:3 * nl] == bytes(nl) + b"\xff" * (2 * nl)
    assert all(f"gcm_nonce16_aad{al}_len32_n1" in by for al in (1, 15, 17, 64))
    assert all(f"gcm_nonce16_aad16_len32_n{n}" in by for n in (255, 256, 257, 513))
    assert "gcm_wrap_len17_n65" in by and "gcm_wrap_len32_n65" in by


def test_spec_vectors_are_the_literals_and_openssl_agrees():
    by = {c["name"]: c for c in G.load()["gcm"]}
    for t, tag in enumerate(SPEC_TAGS, 1):
        c = by[f"gcm_spec_tc{t}"]
        assert G.D.field_bytes(c["tags"]).hex() == tag
        ct, tags = G.expected(c)                           # OpenSSL, held to the literal fields
        assert tags.hex() == tag and len(ct) == c["len"]


def test_wrap_rows_wrap():
    """J0 of the crafted rows ends in 0xFFFFFFFF / 0xFFFFFFFE: the keystream counter wraps to 0 in
    block 1 or 2 while the tag's mask is E_k(J0) itself"""
    for c in (c for c in G.load()["gcm"] if "wrap_rows" in c):
        k, nc = G.D.field_bytes(c["keys"]), G.D.field_bytes(c["nonces"])
        lows = [G.D.gcm_j0(k[16 * i:16 * i + 16], nc[16 * i:16 * i + 16]) & 0xFFFFFFFF for i in range(c["wrap_rows"])]
        assert lows == [0xFFFFFFFF] * 3 + [0xFFFFFFFE] * 3
        assert c["len"] in (17, 32) and c["aad_len"] == 16


def test_seal_is_encrypt_with_the_tag_kept():
    from flamingo_amd import crypto as C
    for c in G.load()["gcm"]:
        nl, al, ln = c["nonce_len"], c["aad_len"], c["len"]
        k, nc, a, d = (G.D.field_bytes(c[f]) for f in ("keys", "nonces", "aad", "data"))
        for i in range(min(c["n"], 4)):
            row = (k[16 * i:16 * i + 16], d[ln * i:ln * i + ln], nc[nl * i:nl * i + nl])
            ct, tag = C.aes_gcm_seal(*row, a[al * i:al * i + al])
            assert len(tag) == 16 and len(ct) == ln
            if ln:                                         # the tag-dropping pair takes no empty message apart
                assert ct == C.aes_gcm_encrypt(*row)[0] and C.aes_gcm_decrypt(row[0], ct, row[2]) == row[1]
            assert C.aes_gcm_open(row[0], ct, tag, row[2], a[al * i:al * i + al]) == row[1]


def test_open_refuses_a_flipped_bit_anywhere():
    from flamingo_amd import crypto as C
    key, nonce, aad, data = bytes(range(16)), bytes(range(16, 32)), b"iteration-dealer", bytes(range(64, 96))
    ct, tag = C.aes_gcm_seal(key, data, nonce, aad)
    assert C.aes_gcm_open(key, ct, tag, nonce, aad) == data
    flip = lambda b, i: b[:i] + bytes([b[i] ^ 1]) + b[i + 1:]  # noqa: E731
    for i in (0, 31):
        assert C.aes_gcm_open(key, flip(ct, i), tag, nonce, aad) is None
    for i in (0, 15):
        assert C.aes_gcm_open(key, ct, flip(tag, i), nonce, aad) is None
        assert C.aes_gcm_open(key, ct, tag, nonce, flip(aad, i)) is None
        assert C.aes_gcm_open(key, ct, tag, flip(nonce, i), aad) is None
        assert C.aes_gcm_open(flip(key, i), ct, tag, nonce, aad) is None
    assert C.aes_gcm_open(key, ct, tag, nonce, b"") is None and C.aes_gcm_open(key, ct, tag, nonce, aad + b"\0") is None
    assert C.aes_gcm_open(key, ct[:-1], tag, nonce, aad) is None and C.aes_gcm_open(key, ct, tag[:15], nonce, aad) is None
    tag0 = C.aes_gcm_seal(key, b"", nonce, aad)[1]          # a tag over the AAD alone
    assert C.aes_gcm_open(key, b"", tag0, nonce, aad) == b"" and C.aes_gcm_open(key, b"", tag0, nonce, b"x") is None


def test_argument_rules_checker(tmp_path):
    """tools/args_check.cpp (flm_call_args.h + the bounce-buffer layout), built without a sanitizer"""
    cxx = next((c for c in ("c++", "g++", "clang++", "hipcc") if shutil.which(c)), None)
    assert cxx, "no C++ compiler"
    exe = str(tmp_path / "args_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-I", os.path.join(ROOT, "flamingo_amd", "csrc"),
                    os.path.join(ROOT, "tools", "args_check.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "all checks passed" in out.stdout, out.stdout + out.stderr


def test_header_declares_and_bindings_name_the_calls():
    from flamingo_amd import _lib
    with open(os.path.join(ROOT, "include", "flamingo_hip.h")) as f:
        hdr = f.read()
    with open(os.path.join(ROOT, "integration", "util_flm.py")) as f:
        util = f.read()
    for name in ("flm_aes_gcm_seal", "flm_aes_gcm_seal_dev", "flm_aes_gcm_open", "flm_aes_gcm_open_dev"):
        assert re.search(r"\bint %s\(" % name, hdr) and name in _lib.SIGNATURES
    # the host-pointer forms have one argument less than the device forms (the stream)
    for host in ("flm_aes_gcm_seal", "flm_aes_gcm_open"):
        assert len(_lib.SIGNATURES[host + "_dev"][1]) == len(_lib.SIGNATURES[host][1]) + 1
        assert '"%s"' % host in util
    assert "def aes_gcm_seal(" in util and "def aes_gcm_open(" in util


@pytest.mark.parametrize("name", ["aes_gcm_seal_wire", "aes_gcm_open_wire", "aes_gcm_seal_dev", "aes_gcm_open_dev"])
def test_engine_has_the_methods(name):
    from flamingo_amd.engine import MaskEngine
    assert callable(getattr(MaskEngine, name))
