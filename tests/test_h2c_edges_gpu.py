"""The tail of hash_to_curve_kernel (flm_p256.hip h2c_tail: mod_n_384, h2c_map, the lane swap, jac_add,
the affine conversion) at inputs no message reaches, byte for byte against the big-int oracle
(oracle/ec_oracle.h2c_from_uniform), through flm_h2c_from_uniform (flm_internal.h): the same device
function on 96 uniform bytes the test chooses.

The cases are tests/h2c_cases.py (premises: tests/test_h2c_cases_cpu.py): every fold count of the
reduction and its carry edges, u = 0 and the roots of 1/10 (den = 0, the sgn0 flip), Montgomery forms
with edge limbs, Q0 = +-Q1 (doubling, infinity), each in both lanes of a pair and at the edges of a
64-lane workgroup (32 rows).  Where the denominator is 0 the reference raises; the kernel and the
oracle take RFC 9380's inv0 there, which these tests pin."""
import ctypes

import numpy as np
import pytest

import ec_oracle as E
import h2c_cases as C

pytestmark = pytest.mark.gpu

GUARD8, GUARD32 = 0xA5, 0x5A5A5A5A
GUARD_ROWS = 3
EINVAL = -1


@pytest.fixture(scope="module")
def eng():
    from flamingo_amd import MaskEngine
    e = MaskEngine(0)
    u8p, u32p = ctypes.POINTER(ctypes.c_uint8), ctypes.POINTER(ctypes.c_uint32)
    fn = e.lib.flm_h2c_from_uniform          # internal: not in the public header nor in _lib.SIGNATURES
    fn.restype = ctypes.c_int
    fn.argtypes = [ctypes.c_void_p, u8p, ctypes.c_int, u8p, u32p]
    yield e
    e.close()


def run(eng, ubs):
    """flm_h2c_from_uniform on the rows ubs -> (rc, out (n, 64), flags (n,)); out and flags carry
    GUARD_ROWS guard rows past n, checked here."""
    from flamingo_amd._lib import p_u8, p_u32
    n = len(ubs)
    uni = np.frombuffer(b"".join(ubs), np.uint8).reshape(n, 96).copy()
    out = np.full((n + GUARD_ROWS, 64), GUARD8, np.uint8)
    fl = np.full(n + GUARD_ROWS, GUARD32, np.uint32)
    rc = eng.lib.flm_h2c_from_uniform(eng.ctx, p_u8(uni), n, p_u8(out), p_u32(fl))
    assert np.all(out[n:] == GUARD8) and np.all(fl[n:] == GUARD32), "wrote past row n"
    return rc, out[:n], fl[:n]


def check(eng, rows, what):
    rc, out, fl = run(eng, [r.ub for r in rows])
    assert rc == 0, (what, eng.lib.flm_last_error(eng.ctx).decode())
    bad = []
    for i, r in enumerate(rows):
        wire, flag = C.expect(r.ub)
        assert flag == (4 if "inf" in r.special else 0)
        if out[i].tobytes() != wire or int(fl[i]) != flag:
            bad.append((i, r.name, sorted(r.special), hex(int(fl[i])), out[i].tobytes().hex()[:16], wire.hex()[:16]))
    assert not bad, (what, len(bad), bad[:8])
    assert not (fl & 8).any()


def test_whole_case_list(eng):
    """Every reduction, map and pair case in one launch: points byte for byte, flags per element
    (bit 2 exactly on the infinity rows, whose bytes are zero; bit 3 never), rc 0."""
    rows = C.rows()
    check(eng, rows, "all cases")
    rc, out, fl = run(eng, [r.ub for r in rows])
    inf = np.array(["inf" in r.special for r in rows])
    assert rc == 0 and inf.sum() == 4
    assert np.array_equal((fl & 4) != 0, inf) and not out[inf].any() and out[~inf].any(axis=1).all()


def test_special_rows_alone(eng):
    """The infinity, u = 0 and den = 0 rows without the others, then one launch each."""
    sp = C.special_rows()
    check(eng, sp, "special rows")
    for r in sp:
        check(eng, [r], r.name)


@pytest.mark.parametrize("n", C.BATCH_SIZES)
def test_batch_edges(eng, n):
    """An infinity pair, a doubling pair and a u = 0 row at row 0, row n - 1 and on both sides of every
    32-row (workgroup) boundary, ordinary rows elsewhere; nothing is written past row n."""
    for rot in range(3):
        check(eng, C.edge_batch(n, rot), (n, rot))


def test_flags_are_per_element(eng):
    """Ordinary rows between infinity rows keep flag 0 and their own point."""
    rows = C.flag_batch()
    check(eng, rows, "alternating infinity rows")
    _, out, fl = run(eng, [r.ub for r in rows])
    assert np.array_equal(fl, np.where(np.arange(len(rows)) % 2 == 0, 4, 0))
    assert len({out[i].tobytes() for i in range(1, len(rows), 2)}) == len(rows) // 2


def test_the_two_kernels_share_one_tail(eng):
    """flm_h2c_from_uniform(expand_message_xmd(msg)) == flm_hash_to_curve(msg), both on the GPU, for the
    messages of test_counter_edges_gpu's every-length test and the decimal strings at the digit edges."""
    g = np.random.Generator(np.random.PCG64(65))
    msgs = [bytes(g.integers(0, 256, ln, dtype=np.uint8)) for ln in range(65)] + [b"\xff" * ln for ln in range(65)]
    msgs += [str(v).encode() for v in (0, 9, 10, 65535)]
    want, wfl = eng.hash_to_curve_wire(msgs)
    rc, out, fl = run(eng, [E.expand_message_xmd(m, E.DST, 96) for m in msgs])
    assert rc == 0 and not fl.any() and not wfl.any()
    assert np.array_equal(out, want), np.flatnonzero((out != want).any(axis=1))[:8]
    dec, _ = eng.hash_to_curve_decimal(65535, 1)
    assert np.array_equal(dec[0], out[-1])


def test_argument_errors(eng):
    from flamingo_amd._lib import p_u8, p_u32
    fn = eng.lib.flm_h2c_from_uniform
    row = C.rows()[0]
    uni = np.frombuffer(row.ub, np.uint8).copy()
    out, fl = np.full(64, GUARD8, np.uint8), np.full(1, GUARD32, np.uint32)
    assert fn(eng.ctx, p_u8(uni), 0, p_u8(out), p_u32(fl)) == 0                 # n = 0: nothing launched
    assert fn(eng.ctx, None, 0, None, None) == 0
    assert fn(None, p_u8(uni), 1, p_u8(out), p_u32(fl)) == EINVAL
    assert fn(eng.ctx, None, 1, p_u8(out), p_u32(fl)) == EINVAL
    assert fn(eng.ctx, p_u8(uni), 1, None, p_u32(fl)) == EINVAL
    assert fn(eng.ctx, p_u8(uni), -1, p_u8(out), p_u32(fl)) == EINVAL
    assert np.all(out == GUARD8) and fl[0] == GUARD32
    assert fn(eng.ctx, p_u8(uni), 1, p_u8(out), None) == 0                      # flags_out is optional
    assert out.tobytes() == C.expect(row.ub)[0]
    check(eng, C.rows()[:5], "the context works after the refusals")
