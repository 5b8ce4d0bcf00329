"""The dealing fixture (tests/golden/deal_golden.json) is sound, and the batched path's draws are
the host path's: no GPU needed.

* the generator re-run in memory equals the committed file;
* every Shamir case with enough distinct points recovers secret mod n through
  seeds.shamir_recover, from its first and from its last T distinct points; T = 1 puts
  secret mod n in every share;
* every AES case decrypts back through crypto.aes_gcm_decrypt;
* protocol._draw_mi's single draw of a client's m_i, coefficients and nonces is the same stream
  as the host path's separate draws (client_agent.sendVectors), value for value.
"""
import importlib.util
import os
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _generator():
    spec = importlib.util.spec_from_file_location("make_deal_golden",
                                                  os.path.join(ROOT, "tests", "golden", "make_deal_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


G = _generator()


@pytest.fixture(scope="module")
def fixture():
    return G.load()


def test_generator_reproduces_the_fixture(fixture):
    assert G.generate() == fixture
    assert os.path.getsize(G.OUT) < 32 * 1024


def _distinct(points):
    seen, out = set(), []
    for x, y in points:
        if x not in seen:
            seen.add(x)
            out.append((x, y))
    return out


def test_shamir_cases_recover_the_secret(fixture):
    from flamingo_amd.abides.flamingo.seeds import P256_N, shamir_recover
    assert int(fixture["n"], 16) == P256_N
    assert sorted((c["T"], c["C"], c["M"]) for c in fixture["shamir"]) == sorted(G.SHAMIR)
    for case in fixture["shamir"]:
        T, C, M, xs = case["T"], case["C"], case["M"], case["xs"]
        co, sh = G.field_bytes(case["coeffs"]), G.expected(case)
        assert len(co) == T * M * 32 and len(sh) == C * M * 32 and all(0 < x < 2**32 for x in xs)
        word = lambda b, k: int.from_bytes(b[32 * k:32 * k + 32], "big")  # noqa: E731
        for i in range(M):
            secret = word(co, i) % P256_N
            pts = [(xs[c], word(sh, c * M + i)) for c in range(C)]
            assert all(y < P256_N for _, y in pts)
            if T == 1:
                assert all(y == secret for _, y in pts)
            d = _distinct(pts)
            if len(d) >= T:
                assert shamir_recover(d[:T]) == secret, (case["name"], i)
                assert shamir_recover(d[-T:]) == secret, (case["name"], i)
    edge = {0, 1, P256_N - 1, P256_N, P256_N + 1, 2**256 - 1}
    seen = {int.from_bytes(G.field_bytes(c["coeffs"])[o:o + 32], "big")
            for c in fixture["shamir"] for o in range(0, c["T"] * c["M"] * 32, 32)}
    assert edge <= seen
    assert {1, 2, 2**32 - 1} <= {x for c in fixture["shamir"] for x in c["xs"]}
    assert any(len(set(c["xs"])) < len(c["xs"]) for c in fixture["shamir"])


def test_aes_cases_decrypt_back(fixture):
    from flamingo_amd import crypto as C
    plain = [c for c in fixture["aes"] if "wrap_rows" not in c]
    assert sorted((c["nonce_len"], c["len"], c["n"]) for c in plain) == \
        sorted([(nl, ln, n) for nl in (12, 16) for ln in G.AES_LENS for n in (1, 65)]
               + [(nl, 32, n) for nl in (12, 16) for n in G.AES_BATCH_NS])
    assert [(c["nonce_len"], c["len"], c["n"]) for c in fixture["aes"] if "wrap_rows" in c] == \
        [(16, ln, G.WRAP_N) for ln in G.WRAP_LENS]
    assert len({c["name"] for c in fixture["aes"]}) == len(fixture["aes"])
    for case in fixture["aes"]:
        nl, ln, n = case["nonce_len"], case["len"], case["n"]
        k, nc, d = (G.field_bytes(case[f]) for f in ("keys", "nonces", "data"))
        out = G.expected(case)
        assert (len(k), len(nc), len(d), len(out)) == (16 * n, nl * n, ln * n, ln * n)
        for i in range(n):
            assert C.aes_gcm_decrypt(k[16 * i:16 * i + 16], out[ln * i:ln * i + ln], nc[nl * i:nl * i + nl]) == \
                d[ln * i:ln * i + ln], (case["name"], i)
    big = [c for c in fixture["aes"] if c["n"] == 65]
    assert all(G.field_bytes(c["keys"])[:32] == bytes(16) + b"\xff" * 16 for c in big)


def _ghash_mul(x: int, h: int) -> int:
    """x * h in GF(2^128), NIST SP 800-38D algorithm 1 on integers (bit 0 = the top bit)."""
    z, v = 0, h
    for i in range(128):
        if x & (1 << (127 - i)):
            z ^= v
        v = (v >> 1) ^ (0xE1000000000000000000000000000000 if v & 1 else 0)
    return z


def _ctr_stream(key: bytes, j0: int, blocks: int, bits: int) -> bytes:
    """E_k(J0 + 1) || ... || E_k(J0 + blocks), the sum taken in the low `bits` bits of J0."""
    mask = (1 << bits) - 1
    return b"".join(G.aes_ecb_block(key, ((j0 & ~mask) | ((j0 + m) & mask)).to_bytes(16, "big"))
                    for m in range(1, blocks + 1))


def test_wrap_cases_wrap_and_discriminate(fixture):
    """The crafted rows of the counter-wrap cases: J0, recomputed from the committed nonce with a plain
    GHASH, is 0x0123456789abcdef_ffffffff || w, and OpenSSL's bytes are the inc32 keystream.

    A row wraps when the counter of its last block, w + ceil(len / 16), passes 0xffffffff.  The low
    words 0xffffffff and 0xfffffffe wrap at every length of the fixture, 0xfffffff0 only at len = 256
    (0xfffffff0 + 2 < 2^32: at len 17 and 32 those three rows run just below the wrap, and there inc32
    and a 128-bit increment must agree); the rows with w = 2^32 - ceil(len / 16) wrap in their last block
    at every length.  Every row that wraps with len >= 32 has expected bytes that differ from the
    keystream of a 128-bit increment of J0, so a kernel that carried out of the low word fails there."""
    wraps = [c for c in fixture["aes"] if "wrap_rows" in c]
    assert [c["len"] for c in wraps] == list(G.WRAP_LENS)
    xor = lambda a, b: bytes(p ^ q for p, q in zip(a, b))  # noqa: E731
    for case in wraps:
        ln, n, rows = case["len"], case["n"], case["wrap_rows"]
        blocks, lows = (ln + 15) // 16, G.wrap_lows(ln)
        assert rows == 3 * len(lows) and lows[:3] == (0xFFFFFFFF, 0xFFFFFFFE, 0xFFFFFFF0)
        k, nc, d = (G.field_bytes(case[f]) for f in ("keys", "nonces", "data"))
        out = G.expected(case)
        assert k[:32] == bytes(16) + b"\xff" * 16
        wrapped = 0
        for i in range(rows):
            key, data, want = k[16 * i:16 * i + 16], d[ln * i:ln * i + ln], out[ln * i:ln * i + ln]
            assert key == (bytes(16), b"\xff" * 16, G.prg(case["keys"]["prg"], 16 * n)[16 * i:16 * i + 16])[i % 3]
            h = int.from_bytes(G.aes_ecb_block(key, bytes(16)), "big")
            j0 = _ghash_mul(_ghash_mul(int.from_bytes(nc[16 * i:16 * i + 16], "big"), h) ^ 128, h)
            w = lows[i // 3]
            assert j0 == (0x0123456789ABCDEFFFFFFFFF << 32) | w, (case["name"], i)
            assert want == xor(data, _ctr_stream(key, j0, blocks, 32)), (case["name"], i)
            wide = xor(data, _ctr_stream(key, j0, blocks, 128))
            if w + blocks >= 1 << 32:
                wrapped += 1
                if ln >= 32:
                    assert want != wide, (case["name"], i)
            else:
                assert (w, ln) in ((0xFFFFFFF0, 17), (0xFFFFFFF0, 32)) and want == wide, (case["name"], i)
        assert wrapped == (rows if ln == 256 else rows - 3), case["name"]


@pytest.mark.parametrize("committee,seed", [(9, 1), (60, 2), (4, 3), (1, 4)])
def test_one_draw_is_the_host_paths_stream(committee, seed):
    """protocol._draw_mi against the draws of the host path in client_agent.sendVectors: m_i (32
    bytes), T - 1 coefficients through _PyRandom (40 bytes mod n each), one 16-byte nonce per
    member -- and the random state ends in the same place."""
    from flamingo_amd.abides.flamingo import protocol
    from flamingo_amd.abides.flamingo.client_agent import _PyRandom
    from flamingo_amd.abides.flamingo.seeds import P256_N
    T = max(1, int(protocol.fraction * committee))
    host = np.random.RandomState(seed)
    mi = bytes(host.randint(0, 256, size=32, dtype=np.uint8))
    rng = _PyRandom(host)
    coeffs = [rng.randrange(P256_N) for _ in range(T - 1)]
    nonces = [bytes(host.randint(0, 256, size=16, dtype=np.uint8)) for _ in range(committee)]
    agent = types.SimpleNamespace(user_committee=set(range(committee)), key_length=32,
                                  random_state=np.random.RandomState(seed))
    assert protocol._draw_mi(agent) == (mi, coeffs, nonces)
    assert agent.random_state.randint(0, 2**31) == host.randint(0, 2**31)
