"""The premises of tests/test_h2c_edges_gpu.py, checked without a GPU: every case of
tests/h2c_cases.py reaches the branch of hash_to_curve_kernel's tail it is listed for (by the oracle
and by the limb model of mod_n_384, tools/h2c_reduce_model.py), the model equals % n, and the
oracle's map_to_curve equals the reference's own on the map family wherever the reference has an
answer (tests/golden/h2c_map_golden.json, made by tests/golden/make_h2c_map_golden.py)."""
import json
import os
import random
import subprocess
import sys

import pytest

import ec_oracle as E
import h2c_cases as C
import h2c_reduce_model as M

HERE = os.path.dirname(os.path.abspath(__file__))
P, N = E.P, E.N


# ------------------------------------------------------------------ the reduction and its model
def test_model_equals_mod_n_on_cases_and_random_inputs():
    for name, v in C.reduction_values():
        assert M.reduce(v)[0] == v % N, name
    for name, v in C.map_values():
        assert M.reduce(v)[0] == v % N, name
    h = M.histogram(20000, seed=384)                  # asserts reduce(v) == v % n on each
    assert set(h) == {4, 5} and min(h.values()) > 8000, h


def test_fold_bound_and_a_case_for_every_fold_count():
    chain = M.fold_bound()
    assert len(chain) - 1 == M.MAX_FOLDS == 5 <= M.ITERATIONS
    assert chain[-1] < 2**256 <= chain[-2]
    assert [T >> 256 for T in chain[1:]] == [0xffffffff0000000000000001, 0xfffffffe00000002, 0xfffffffe, 1, 0]
    assert sorted(M.FOLD_WITNESSES) == list(range(M.MAX_FOLDS + 1))
    for k, v in M.FOLD_WITNESSES.items():
        assert M.reduce(v) == (v % N, k), k
    counts = {M.reduce(v)[1] for _, v in C.reduction_values()}
    assert counts == set(range(M.MAX_FOLDS + 1))
    # fewer iterations than folds leave the high limbs set: the model's own assertion notices
    with pytest.raises(AssertionError):
        M.reduce(M.FOLD_WITNESSES[5], iterations=4)
    assert M.reduce(M.FOLD_WITNESSES[5], iterations=5) == (M.FOLD_WITNESSES[5] % N, 5)


def test_model_has_the_kernels_constants_and_loop_count():
    """The model replays mod_n_384 as written: its kNc limbs and its loop count are read from the
    source.  No input tells seven iterations from six or five (the bound), so the count is held here."""
    import re
    with open(os.path.join(os.path.dirname(HERE), "flamingo_amd", "csrc", "flm_p256.hip")) as f:
        src = f.read()
    knc = re.search(r"kNc\[7\] = \{([^}]*)\}", src).group(1)
    assert [int(w.strip().rstrip("u"), 16) for w in knc.split(",")] == M.NC_LIMBS
    assert M.NC == 2**256 - N == C.NC < 2**224
    body = src[src.index("__device__ Fe mod_n_384("):src.index("// Montgomery-form inverse by binary GCD")]
    assert [int(x) for x in re.findall(r"for \(int it = 0; it < (\d+); \+\+it\)", body)] == [M.ITERATIONS]
    assert M.ITERATIONS >= M.MAX_FOLDS


def test_reduction_family_holds_what_it_lists():
    vals = dict(C.reduction_values())
    assert len(set(vals.values())) == len(vals) >= 90 and all(0 <= v < 2**384 for v in vals.values())
    for k in (2, 3, 2**32, 2**64, 2**96, 2**128 - 1, C.KMAX):
        assert {k * N - 1, k * N, k * N + 1} & set(vals.values()) == {v for v in (k * N - 1, k * N, k * N + 1) if v < 2**384}
    assert C.KMAX * N < 2**384 <= (C.KMAX + 1) * N and C.KMAX * N + 1 in vals.values()
    assert {0, N, 2**384 - 1, 2**384 - 2, 2**352, 2**384 - 2**352, (2**32 - 1) << 352} <= set(vals.values())
    # a late carry back into limb 8: hi = 1 and lo + Nc crosses 2^256 exactly at lo = 2^256 - Nc
    assert M.reduce(1 << 256 | (2**256 - C.NC - 1))[1] == 1
    assert M.reduce(1 << 256 | (2**256 - C.NC))[1] == 2
    assert M.reduce((2**128 - 1) << 256 | (2**256 - 1))[1] == 5


# ------------------------------------------------------------------ the map
def test_roots_of_one_tenth():
    for s in C.ROOTS:
        assert 0 < s < N and 10 * s * s % P == 1
    assert C.S_PLUS + C.S_MINUS == P and P - N < min(C.ROOTS)


def test_map_family_reaches_its_branches():
    vals = C.map_values()
    us = [v % N for _, v in vals]
    assert [u for u in us[:3]] == [0, 0, 0] and [v for _, v in vals[:3]] == [0, N, C.KMAX * N]
    den0 = [u for u in us if C.map_trace(u).den0]
    assert sorted(set(den0)) == sorted({0, C.S_PLUS, C.S_MINUS}) and len(den0) == 5
    flips = [u for u in us if C.map_trace(u).flip]
    assert set(flips) == {0} and len(flips) == 3                      # the sgn0 flip: u = 0 alone
    for u in us:
        t = C.map_trace(u)
        assert E.on_curve(t.point) and t.point[1] != 0
        assert t.point[0] == C.B30 if t.den0 else t.point[0] != C.B30
    # the b/30 branch: map(0) = (b/30, -r), map(+-sqrt(1/10)) = (b/30, +r) with r the first root
    r = pow((C.B30 ** 3 + E.A * C.B30 + E.B) % P, (P + 1) // 4, P)
    assert r * r % P == (C.B30 ** 3 + E.A * C.B30 + E.B) % P
    assert E.map_to_curve(0) == (C.B30, P - r)
    assert E.map_to_curve(C.S_PLUS) == E.map_to_curve(C.S_MINUS) == (C.B30, r)
    # Montgomery forms with edge limbs, all below n
    for (name, k), (_, v) in zip(C.MONT_K, vals[10:18]):
        assert v < N and v * C.R % P == k, name
    for u in (1, 2, N - 1, P - N + 5, N - (P - N + 5)):
        assert u in us
    # both roots: g(x1) a square for at least a quarter of the random u, a non-square for a quarter
    rnd = C.random_us()
    first = sum(1 for u in rnd if C.map_trace(u).root == 1)
    assert len(rnd) == 64 and 16 <= first <= 48, first
    assert {C.map_trace(u).root for u in us[:18]} == {1, 2}
    big = random.Random(5)
    share = sum(1 for _ in range(2000) if C.map_trace(big.randrange(1, N)).root == 1) / 2000
    assert 0.45 < share < 0.55, share


# ------------------------------------------------------------------ the pairs and the rows
def test_pair_family_reaches_doubling_and_infinity():
    for u in C.doubling_us():
        assert P - N < u < N and P - u < N and not C.map_trace(u).den0
    kinds = [k for *_, k in C.pair_values()]
    assert kinds.count("inf") == 4 and kinds.count("double") == 14
    for name, v0, v1, kind in C.pair_values():
        q0, q1 = E.map_to_curve(v0 % N), E.map_to_curve(v1 % N)
        row = C.make_row(name, v0, v1)
        if kind == "inf":
            assert q0 == E.neg(q1) and E.add(q0, q1) is None and "inf" in row.special, name
            assert C.expect(row.ub) == (bytes(64), 4)
        else:
            assert q0 == q1 and "double" in row.special, name
            assert C.expect(row.ub) == (E.wire(E.mul(2, q0)), 0), name
    # doublings on the b/30 branch and off it
    assert sum(1 for n_, v0, v1, k in C.pair_values() if k == "double" and C.map_trace(v0 % N).den0) == 5


def test_rows_cover_both_lanes_and_their_tags_hold():
    rows = C.rows()
    assert 250 <= len(rows) <= 400 and all(len(r.ub) == 96 for r in rows)
    assert len({r.name for r in rows}) == len(rows)
    for r in rows:
        assert r.u0 == int.from_bytes(r.ub[:48], "big") % N and r.u1 == int.from_bytes(r.ub[48:], "big") % N
        wire, fl = C.expect(r.ub)
        assert (fl == 4) == ("inf" in r.special) == (wire == bytes(64)), r.name
    # every map value in the even lane and in the odd lane, beside an ordinary half
    for name, v in C.map_values():
        h = C.half(v)
        assert any(r.ub[:48] == h and not r.ub[48:] == h for r in rows), name
        assert any(r.ub[48:] == h and not r.ub[:48] == h for r in rows), name
    # every reduction value in some half; every fold count in both
    for name, v in C.reduction_values():
        assert any(C.half(v) in (r.ub[:48], r.ub[48:]) for r in rows), name
    for k, v in M.FOLD_WITNESSES.items():
        assert any(r.ub[:48] == C.half(v) for r in rows) and any(r.ub[48:] == C.half(v) for r in rows), k
    sp = C.special_rows()
    assert sum("inf" in r.special for r in sp) == 4 and sum("zero" in r.special for r in sp) >= 10
    assert all(r.special & {"inf", "zero", "den0"} for r in sp) and 20 <= len(sp) < len(rows) // 4
    # an ordinary half is ordinary
    for k in (0, 1, 1000, 5000, 6000, 8500):
        t = C.map_trace(C.ordinary(k) % N)
        assert not t.den0 and not t.flip


def test_edge_batches_put_every_kind_at_every_edge():
    assert C.edge_positions(1) == [0] and C.edge_positions(2) == [0, 1]
    assert C.edge_positions(33) == [0, 31, 32] and C.edge_positions(64) == [0, 31, 32, 63]
    assert C.edge_positions(129) == [0, 31, 32, 63, 64, 95, 96, 127, 128]
    inf, dbl, zero = C.edge_kinds()
    assert inf.special == {"inf", "zero", "den0"} and dbl.special == {"double"} and zero.special == {"zero", "den0"}
    assert zero.u1 == 0 and zero.u0 != 0
    for n in C.BATCH_SIZES:
        for i in C.edge_positions(n):
            assert {C.edge_batch(n, rot)[i].name for rot in range(3)} == {inf.name, dbl.name, zero.name}
        b = C.edge_batch(n, 0)
        assert len(b) == n and all(not r.special for i, r in enumerate(b) if i not in C.edge_positions(n))
    fb = C.flag_batch()
    assert len(fb) == 67 and all(("inf" in r.special) == (i % 2 == 0) for i, r in enumerate(fb))
    assert len({r.name for r in fb[::2]}) == 4


def test_h2c_from_uniform_is_hash_str_to_curve_after_the_expander():
    for msg in (b"", b"0", b"65535", bytes(range(64))):
        assert E.h2c_from_uniform(E.expand_message_xmd(msg, E.DST, 96)) == E.hash_str_to_curve(msg)


# ------------------------------------------------------------------ the reference as judge
def _golden():
    with open(os.path.join(HERE, "golden", "h2c_map_golden.json")) as f:
        return json.load(f)


def test_oracle_map_matches_the_reference_on_the_map_family():
    g = _golden()
    want = {v % N for _, v in C.map_values()}
    assert {int(p["u"], 16) for p in g["points"]} | {int(r["u"], 16) for r in g["raises"]} == want
    assert len(g["points"]) == len(want) - 3
    for p in g["points"]:
        assert E.map_to_curve(int(p["u"], 16)) == (int(p["x"], 16), int(p["y"], 16)), p["name"]
    # where the denominator is 0 the reference raises: no answer to compare with, inv0 is this project's
    assert sorted(int(r["u"], 16) for r in g["raises"]) == sorted({0, C.S_PLUS, C.S_MINUS})
    assert all(C.map_trace(int(r["u"], 16)).den0 for r in g["raises"])


def test_map_golden_regenerates_from_the_reference():
    """Runs the generator (its own process: it installs stand-in modules) when the reference is there."""
    gen = os.path.join(HERE, "golden", "make_h2c_map_golden.py")
    sys.path.insert(0, os.path.join(HERE, "golden"))
    try:
        import make_h2c_map_golden as G
    finally:
        sys.path.pop(0)
    if not os.path.isdir(os.path.join(G.REF, "util", "crypto")):
        pytest.skip("the reference is not on this machine")
    out = subprocess.run([sys.executable, gen, "--print"], check=True, capture_output=True, text=True).stdout
    assert json.loads(out) == _golden()
