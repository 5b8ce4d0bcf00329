"""The premises of tests/test_feldman_gpu.py, checked without a GPU: every case of
tests/feldman_cases.py reaches the exceptional addition it is listed for (recomputed over the
exponents, not assumed), its claimed verdict and flags are what the reference's power-sum form
gives (feldman_cases.expected), and the host twin crypto.feldman_verify returns every one of these
verdicts and every verdict the reference itself recorded (tests/golden/dkg_golden.json)."""
import importlib.util
import os
import re
import shutil
import subprocess

import pytest

import ec_oracle as E
import feldman_cases as F
from flamingo_amd import crypto

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = E.N


def _generator():
    spec = importlib.util.spec_from_file_location("make_dkg_golden",
                                                  os.path.join(ROOT, "tests", "golden", "make_dkg_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


G = _generator()


def _pts(com):
    """Wire commitments as crypto.feldman_verify takes them: (x, y) pairs, None for 64 zero bytes.
    An invalid one stays a pair: refusing it is the function's job."""
    return [None if b == F.INF else (int.from_bytes(b[:32], "big"), int.from_bytes(b[32:], "big")) for b in com]


def test_case_names_are_unique_and_every_shape_is_there():
    assert len(F.BY_NAME) == len(F.CASES)
    assert set(F.groups()) == {(1, 6), (2, 6), (3, 6), (3, 32)}


@pytest.mark.parametrize("case", F.CASES, ids=lambda c: c.name)
def test_claimed_result_is_the_power_sums(case):
    ok, flags, point = F.expected(case.com, case.x, case.x_bits, case.share)
    assert (ok, flags) == (case.ok, case.flags)
    if case.coeffs is not None and not case.x >> case.x_bits:
        # commitments are c_k G: F(x) = f(x) G, and a share below n passes iff it is f(x)
        f = F.poly(case.coeffs, case.x)
        assert point == E.wire(E.mul(f))
        assert case.ok == (case.share == f)
        assert bool(flags & F.F_INF) == (f == 0)


def test_exceptional_additions_are_reached():
    ev = lambda name: F.horner_events(F.BY_NAME[name].coeffs, F.BY_NAME[name].x, F.BY_NAME[name].x_bits)  # noqa: E731
    # every multiplication's first set bit adds into R at infinity
    assert (0, 5, "inf") in ev("final_double")
    # P + P and P - P in the last addition
    assert (0, "term", "double") in ev("final_double")
    assert (0, "term", "cancel") in ev("f_inf_share0")
    # the accumulator is at infinity after term 1, so term 0's multiplication adds nothing
    mid = ev("mid_inf")
    assert (1, "term", "cancel") in mid and (0, "term", "inf") in mid
    assert not [e for e in mid if e[0] == 0 and e[1] != "term"] or all(e[2] == "inf" for e in mid if e[0] == 0)
    # infinity commitments as the top, the middle and the constant term
    assert (1, "term", "inf") in ev("inf_top") and (1, "term", "inf") in ev("inf_mid")
    assert (0, "term", "inf") in ev("inf_const")
    # x = 0 walks no set bit: each term is added to infinity
    assert ev("x0") == [(1, "term", "inf"), (0, "term", "inf")]
    # and the ordinary cases meet nothing but the first-bit additions
    for name in ("x_max", "share_1", "share_n_minus_1", "x_at_bits_edge"):
        assert all(kind == "inf" and where != "term" for _, where, kind in ev(name)), name


def test_share_cases_cover_the_listed_values():
    vals = {c.share for c in F.CASES if c.name.startswith("share_")}
    assert vals == {1, 2, 3, 15, 16, 17, 1 << 255, N - 2, N - 1, N, N + 1, (1 << 256) - 1}
    for c in F.CASES:
        if c.share >= N:
            assert not c.ok and c.flags & F.F_SHARE
            # refused, not reduced: the reduced share would pass
            assert F.expected(c.com, c.x, c.x_bits, c.share % N)[0]


def test_invalid_commitments_are_invalid_for_the_listed_reason():
    for k in range(3):
        c = F.BY_NAME[f"flip_y_term{k}"]
        pt = _pts(c.com)[k]
        assert pt[0] < E.P and pt[1] < E.P and not E.on_curve(pt)
    assert _pts(F.BY_NAME["x_is_p"].com)[1][0] == E.P
    assert _pts(F.BY_NAME["y_is_p"].com)[0][1] == E.P
    c = F.BY_NAME["x_over_bits"]
    assert c.x >> c.x_bits and c.share == F.poly(c.coeffs, c.x) and c.flags == F.F_XBITS


def test_pool_alternates_valid_and_invalid_rows():
    rows, res = F.pool()
    assert len(rows) >= 32 and all(len(com) == F.POOL_T for com, _, _ in rows)
    assert [r[0] for r in res] == [i % 2 == 0 for i in range(len(rows))]


@pytest.mark.parametrize("case", [c for c in F.CASES if not c.x >> c.x_bits], ids=lambda c: c.name)
def test_host_twin_on_edge_cases(case):
    assert crypto.feldman_verify(case.share, case.x, _pts(case.com)) == case.ok


def test_host_twin_refuses_what_has_no_wire_form():
    c = F.BY_NAME["share_1"]
    assert crypto.feldman_verify(c.share, c.x, _pts(c.com))
    assert not crypto.feldman_verify(-1, c.x, _pts(c.com))
    assert not crypto.feldman_verify(1 << 256, c.x, _pts(c.com))
    assert not crypto.feldman_verify(c.share, -1, _pts(c.com))
    assert crypto.feldman_point(c.x, _pts(c.com)) == E.mul(c.share)
    assert crypto.feldman_point(5, []) is None and crypto.feldman_verify(0, 5, [])


def test_host_twin_on_the_references_verdicts():
    fixture = G.load()
    seen = {}
    for n, T, com, x, share, ok, label in G.rows(fixture):
        assert len(com) == T == int(n / 3) + 2
        assert crypto.feldman_verify(int.from_bytes(share, "big"), x, _pts(com)) == ok, label
        kind = label.rsplit("-", 1)[1]
        seen[(n, kind, ok)] = seen.get((n, kind, ok), 0) + 1
    # the reference accepts every honest row and refuses every tampered one
    assert seen == {(n, kind, kind == "honest"): cnt for n, cnt in ((6, 36), (60, 12))
                    for kind in ("honest", "share+1", "wrong_id", "swap")}


def test_oracle_agrees_with_the_references_verdicts():
    for n, T, com, x, share, ok, label in G.rows(G.load()):
        assert F.expected(com, x, max(1, n.bit_length()), int.from_bytes(share, "big"))[0] == ok, label


def test_generator_replays_the_fixture():
    if not os.path.isdir(os.path.join(G.REF, "agent", "dkg")):
        pytest.skip("the reference is not on this machine")
    assert G.generate() == G.load()
    assert os.path.getsize(G.OUT) < 64 * 1024


# ------------------------------------------------------------------ the argument rules and the ABI
def test_argument_rules_checker(tmp_path):
    """tools/args_check.cpp (flm_call_args.h + the bounce-buffer layout), built without a sanitizer"""
    cxx = next((c for c in ("c++", "g++", "clang++", "hipcc") if shutil.which(c)), None)
    assert cxx, "no C++ compiler"
    exe = str(tmp_path / "args_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-I", os.path.join(ROOT, "flamingo_amd", "csrc"),
                    os.path.join(ROOT, "tools", "args_check.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "all checks passed" in out.stdout, out.stdout + out.stderr


def test_header_declares_and_library_binds_the_calls():
    from flamingo_amd import _lib
    with open(os.path.join(ROOT, "include", "flamingo_hip.h")) as f:
        hdr = f.read()
    for name in ("flm_feldman_verify", "flm_feldman_verify_dev"):
        assert re.search(r"\bint %s\(" % name, hdr) and name in _lib.SIGNATURES
    assert "agent/dkg/SA_ClientAgent.py:219-228" in hdr
    # the fixed-base half is written once and called by both kernels
    with open(os.path.join(ROOT, "flamingo_amd", "csrc", "flm_p256.hip")) as f:
        src = f.read()
    assert src.count("Jac fixed_base_step(") == 1 and src.count("fixed_base_step(") == 3
    assert src.count("kGOdd[t]") == 2          # the table is read in fixed_base_add alone
