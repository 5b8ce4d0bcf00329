"""The 256-bit field layers (flamingo_amd/csrc/flm_fe256.h, flm_fe_row.h, wnaf5 of flm_jac256.h) one
operation at a time on the GPU, bit for bit against Python integers, on the lists of
tests/fe_cases.py (premises: tests/test_fe_cases_cpu.py): all pairs of ~30 edge values and 2,000
random pairs per modulus, operands solved so that the value before the last conditional subtraction
lies in [m, 2^256) or on 2^256, witnesses for every carry event of fe_sqr and every carry count of
fe_mul's columns, the row field's many-pass operands in every row position of a wave, lazy values
in [p, 2^256) through row::canon and row::is_zero.

The operations run through the test-only harness tests/fieldtest/flm_fieldtest.hip, which
flamingo_amd.build compiles into flamingo_amd/lib/libflm_fieldtest.so (a missing library fails these
tests).  Limit of the harness: it includes the product's headers unchanged but compiles its own
copies of the inlined device functions, so it tests the source of the layers, not the product
library's code objects.  The last two tests therefore drive the product's own shamir_combine_kernel
and shamir_deal_kernel, whose entry points give control of sc_mul's operands, into the same window.

torch is imported before the harness is loaded: one HIP runtime per process."""
from __future__ import annotations

import ctypes
import os

import numpy as np
import pytest

import fe_cases as F

pytestmark = pytest.mark.gpu

P, N, R = F.P, F.N, F.R
R_INV = {m: pow(R, -1, m) for m in (P, N)}
OPS = {"fe_mul": 0, "fe_sqr": 1, "fe_add": 2, "fe_sub": 3, "fe_neg": 4, "to_mont": 5, "from_mont": 6, "fe_is_zero": 7,
       "fe_eq": 8, "fe_lt_p": 9, "sc_mul": 10, "sc_add": 11, "sc_below_n": 12, "sc_lt_n": 13, "wnaf5": 14,
       "row_mul": 20, "row_sqr": 21, "row_add": 22, "row_sub": 23, "row_neg": 24, "row_canon": 25, "row_is_zero": 26}
NAF_WORDS = 65


@pytest.fixture(scope="module")
def run():
    import torch  # noqa: F401  (first: the harness shares its HIP runtime)
    from flamingo_amd import build
    path = os.environ.get("FLM_FIELDTEST_LIB", build.FIELDTEST_OUT)      # another build of the harness, as FLM_LIB_PATH
    assert os.path.exists(path), f"{path} is missing: flamingo_amd.build.build() makes libflm_fieldtest.so"
    lib = ctypes.CDLL(path)
    fn = lib.flm_fieldtest_run
    u32p = ctypes.POINTER(ctypes.c_uint32)
    fn.restype = ctypes.c_int
    fn.argtypes = [ctypes.c_int, u32p, u32p, u32p, ctypes.c_int, ctypes.c_int]

    def call(op: str, a, b=None) -> np.ndarray:
        """one launch of `op` on the integers a (and b) -> (n, words) uint32"""
        n = len(a)
        words = 16 if op.startswith("row_") else NAF_WORDS if op == "wnaf5" else 8
        wa = pack(a)
        wb = pack(b) if b is not None else None
        out = np.full((n, words), 0xA5A5A5A5, np.uint32)
        rc = fn(OPS[op], wa.ctypes.data_as(u32p), wb.ctypes.data_as(u32p) if wb is not None else None,
                out.ctypes.data_as(u32p), n, 0)
        assert rc == 0, f"{op}: HIP error {rc}"
        return out

    return call


def pack(xs) -> np.ndarray:
    """integers below 2^256 -> (n, 8) little-endian uint32 limbs"""
    return np.frombuffer(b"".join(int(x).to_bytes(32, "little") for x in xs), "<u4").reshape(len(xs), 8).copy()


def unpack(rows: np.ndarray) -> list:
    return [int.from_bytes(r.astype("<u4").tobytes(), "little") for r in rows]


def check(run, op: str, a, b, expect):
    """the launch's results against the integers `expect`; the first mismatch with its operands in hex"""
    a, expect = list(a), list(expect)
    b = list(b) if b is not None else None
    assert len(a) == len(expect) and (b is None or len(b) == len(a))
    got = run(op, a, b)
    want = pack(expect)
    if op.startswith("row_"):
        want = np.concatenate([want, np.zeros_like(want)], axis=1)       # lanes 8..15 hold 0
    bad = np.flatnonzero((got != want).any(axis=1))
    if bad.size:
        i = int(bad[0])
        print(f"{op}: {bad.size} of {len(a)} differ; first at element {i}:\n  a = {a[i]:#066x}" +
              (f"\n  b = {b[i]:#066x}" if b is not None else "") +
              f"\n  got    {[f'{w:08x}' for w in got[i]]}\n  expect {[f'{w:08x}' for w in want[i]]}")
    assert bad.size == 0, f"{op}: {bad.size} of {len(a)} results differ from the integers (first: element {int(bad[0])})"


def split(pairs):
    pairs = list(pairs)
    return [a for a, _ in pairs], [b for _, b in pairs]


# ------------------------------------------------------------------ the lane field mod p
def test_fe_mul(run):
    """all structured and random pairs, the largest and the zero carry count of every column, and
    T on every window target (a selection on the ninth word alone returns T there, not T - p)"""
    pairs = list(F.structured_pairs(P)) + [(a, b) for _, _, a, b, _ in F.mul_count_cases()] + \
        [(a, b) for _, _, a, b in F.mul_window_cases(P)]
    pairs += [(b, a) for a, b in pairs[-len(F.mul_window_cases(P)):]]
    a, b = split(pairs)
    check(run, "fe_mul", a, b, [x * y * R_INV[P] % P for x, y in pairs])


def test_fe_sqr(run):
    """structured and random values, a witness of every reachable carry event in every column, and
    squares whose T lies in the window and on 2^256, 2^256 + 1"""
    a = list(F.unary_values(P)) + [x for _, _, x in F.sqr_event_cases()] + \
        [x for _, _, x in F.sqr_window_cases() if x is not None] + [0x80000001FFFFFFFE]
    check(run, "fe_sqr", a, None, [x * x * R_INV[P] % P for x in a])
    # the same values as products: fe_mul(a, a) takes the general columns
    check(run, "fe_mul", a, a, [x * x * R_INV[P] % P for x in a])


def test_to_mont_and_from_mont(run):
    a = list(F.unary_values(P)) + [x for _, _, x in F.to_mont_window_cases(P) if x is not None]
    check(run, "to_mont", a, None, [x * R % P for x in a])
    a = list(F.from_mont_values())
    check(run, "from_mont", a, None, [x * R_INV[P] % P for x in a])


def test_fe_add_sub_neg(run):
    pairs = list(F.structured_pairs(P)) + list(F.add_edge_cases(P)) + list(F.sub_edge_cases(P))
    a, b = split(pairs)
    check(run, "fe_add", a, b, [(x + y) % P for x, y in pairs])
    check(run, "fe_sub", a, b, [(x - y) % P for x, y in pairs])
    a = list(F.unary_values(P))
    assert a[0] == 0
    check(run, "fe_neg", a, None, [-x % P for x in a])


def test_fe_predicates(run):
    v = list(F.range_values(P))
    check(run, "fe_lt_p", v, None, [int(x < P) for x in v])
    check(run, "fe_is_zero", v, None, [int(x == 0) for x in v])
    # equal values, and values that differ in the lowest or the highest bit of one limb only
    pairs = list(F.structured_pairs(P)[:len(F.structured_values(P)) ** 2]) + [(x, x) for x in v]
    pairs += [(x, x ^ (1 << (32 * k + j))) for x in v[:40] for k in range(8) for j in (0, 31)]
    a, b = split(pairs)
    check(run, "fe_eq", a, b, [int(x == y) for x, y in pairs])


# ------------------------------------------------------------------ the scalar field mod n
def test_sc_mul(run):
    """as fe_mul, with the entry into Montgomery form (b = R^2 mod n) on its window targets and the
    unreduced first operands a = n (T = n exactly: result 0), n + 1 and 2^256 - 1"""
    r2 = R * R % N
    pairs = list(F.structured_pairs(N)) + [(a, b) for _, _, a, b in F.mul_window_cases(N)] + \
        [(b, a) for _, _, a, b in F.mul_window_cases(N)] + \
        [(a, r2) for _, _, a in F.to_mont_window_cases(N) if a is not None] + list(F.sc_mul_unreduced_cases())
    a, b = split(pairs)
    check(run, "sc_mul", a, b, [x * y * R_INV[N] % N for x, y in pairs])


def test_sc_add_below_n_lt_n(run):
    pairs = list(F.structured_pairs(N)) + list(F.add_edge_cases(N))
    a, b = split(pairs)
    check(run, "sc_add", a, b, [(x + y) % N for x, y in pairs])
    v = list(F.range_values(N))
    check(run, "sc_below_n", v, None, [x - N if x >= N else x for x in v])
    check(run, "sc_lt_n", v, None, [int(x < N) for x in v])


def test_wnaf5(run):
    ks = list(F.wnaf_scalars())
    be = [int.from_bytes(int(k).to_bytes(32, "big"), "little") for k in ks]      # the words hold big-endian bytes
    got = run("wnaf5", be).view(np.int8).reshape(len(ks), NAF_WORDS * 4)
    want = np.array([F.EC.naf5(k) + [0, 0] for k in ks], np.int8)
    bad = np.flatnonzero((got != want).any(axis=1))
    assert bad.size == 0, f"wnaf5 differs at k = {ks[int(bad[0])]:#x}"


# ------------------------------------------------------------------ the row field
def test_row_mul_sqr(run):
    """lazy results bit for bit as the model's (operands anywhere in [0, 2^256)); the first 16
    elements put the pair with the most carry passes in each row position of a wave, beside a
    one-pass pair, zero and p, whose extra passes must change nothing"""
    pairs = list(F.row_pairs("mul"))
    a, b = split(pairs)
    check(run, "row_mul", a, b, [F.row_expect("mul", x, y) for x, y in pairs])
    a = list(F.row_values("sqr"))
    check(run, "row_sqr", a, None, [F.row_expect("sqr", x) for x in a])


def test_row_add_sub_neg(run):
    for op in ("add", "sub"):
        pairs = list(F.row_pairs(op))
        a, b = split(pairs)
        check(run, "row_" + op, a, b, [F.row_expect(op, x, y) for x, y in pairs])
    a = list(F.row_values("neg"))
    check(run, "row_neg", a, None, [F.row_expect("neg", x) for x in a])


def test_row_canon_is_zero(run):
    a = list(F.row_values("canon"))
    assert [F.row_expect("canon", x) for x in a] == [x % P for x in a]
    check(run, "row_canon", a, None, [x % P for x in a])
    a = list(F.row_values("is_zero"))
    got = run("row_is_zero", a)
    want = np.array([[int(x % P == 0)] * 16 for x in a], np.uint32)      # the verdict in every lane of the row
    bad = np.flatnonzero((got != want).any(axis=1))
    assert bad.size == 0, f"row_is_zero differs at a = {a[int(bad[0])]:#x}: {got[int(bad[0])]}"
    # a short list whose last wave is padded: 1, 2 and 3 elements
    for n in (1, 2, 3):
        check(run, "row_canon", [R - 1, P, P + 1][:n], None, [R - 1 - P, 0, 1][:n])


# ------------------------------------------------------------------ the product's own kernels
@pytest.fixture(scope="module")
def eng():
    from flamingo_amd import MaskEngine
    e = MaskEngine(0)
    yield e
    e.close()


def test_shamir_combine_in_the_window(eng):
    """T = 1: lambda with sc_mul(lambda, R^2 mod n) in the window (and one on 2^256 + 1), shares y with
    the second product in the window or at T >= 2^256; plain and unreduced y beside them"""
    extra = (1, 2, N - 1, N, N + 1, R - 1, 0x1234567 << 200)
    bad = []
    for name, _, lam in F.combine_lambda_cases():
        ys = [y for _, _, y in F.combine_share_cases(lam)] + list(extra)
        got = eng.shamir_combine([ys], [lam])
        bad += [(name, hex(lam), hex(y)) for y, g in zip(ys, got) if g != (lam * y % N).to_bytes(32, "big")]
    if bad:
        print("first mismatch (lambda target, lambda, y):", bad[0])
    assert bad == []


def test_shamir_deal_in_the_window(eng):
    """T = 2: y = c1 x + c0 with the top coefficient solved so that sc_mul(c1, x R mod n) has T on
    every reachable target for x = 2 and x = 2^32 - 1 (none is reachable for x = 1, which runs too)"""
    c1 = [c for x in F.DEAL_XS for _, _, c in F.deal_cases(x)]
    c0 = [(7 * c + 1) % N for c in c1]
    c0[:3] = [0, N - 1, R - 1]
    got = eng.shamir_deal([c0, c1], list(F.DEAL_XS))
    bad = [(x, hex(a), hex(b)) for x, row in zip(F.DEAL_XS, got) for a, b, g in zip(c1, c0, row) if g != (a * x + b) % N]
    if bad:
        print("first mismatch (x, c1, c0):", bad[0])
    assert bad == []
