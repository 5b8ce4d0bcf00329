"""The GPU inversion (flm_fe256.h inv_bingcd) and ecdsa_verify_kernel's joint ladder at the branches
tests/inv_cases.py steers them into (premises: tests/test_inv_cases_cpu.py), every comparison exact:
verdicts, flags, bytes.

* mod n, through flm_ecdsa_verify and flm_ecdsa_verify_dev: valid signatures whose s needs 15 to 18
  outer steps, takes the nga / ngb negation, puts a bg_lin_modp quotient in each of its four ranges
  and starts a window at every aligned limb; each with a twin whose digest has one bit flipped.
* mod p, through flm_h2c_from_uniform (flm_internal.h), the den that h2c_map inverts: 15 to 18
  steps and the negations at outer steps 1 to 9, in both lanes of a pair, against
  oracle/ec_oracle.h2c_from_uniform byte for byte.
* the ladder: valid signatures under keys solved so that the accumulator equals the addend, or its
  negative, at the G and at the Q addition of windows 0, 1, 31, 62 and 63, and carries on from
  infinity.

Each family runs as one batch, every row alone, and at the rows on both sides of a workgroup
boundary among ordinary rows.

What these cannot tell (tests/inv_cases.py has the detail): a verdict does not see the sign of
s^-1, since x(-R) = x(R), so the mod-n rows pin it up to sign and the den rows pin the sign; and
every known input has its result after 17 of the 18 outer steps, so a 16-step kernel fails here
and a 17-step kernel would not.

Not driven from here, because no input of a public call sets it: the Z that ec_finish_kernel and
feldman_verify_kernel invert, and h2c_tail's R.Z.  They call the same fe_inv_bingcd source; the den
path above is the mod-p instance that can be steered."""
from __future__ import annotations

import ctypes

import numpy as np
import pytest

import inv_cases as C

pytestmark = pytest.mark.gpu

GUARD = 64
GUARD8, GUARD32, GUARD_ROWS = 0xA5, 0x5A5A5A5A, 3


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


# ------------------------------------------------------------------ flm_ecdsa_verify, both forms
def _rows(cases):
    hexrows = lambda k, n: np.frombuffer(b"".join(bytes.fromhex(c[k]) for c in cases), np.uint8).reshape(-1, n)  # noqa: E731
    sig = np.concatenate([hexrows("r", 32), hexrows("s", 32)], axis=1)
    return hexrows("q", 64).copy(), hexrows("e", 32).copy(), np.ascontiguousarray(sig)


def _guarded(nbytes):
    """A device byte buffer of nbytes followed by GUARD bytes of 0xA5 -> (whole, payload view)."""
    import torch
    whole = torch.full((nbytes + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    return whole, whole[:nbytes]


def _dev_verify(eng, q, e, sig):
    """the *_dev call on guarded outputs -> (ok, flags); the guards are checked here"""
    import torch
    n = q.shape[0]
    dq, de, ds = (torch.from_numpy(a).cuda() for a in (q, e, sig))
    ok_whole, ok = _guarded(n)
    fl_whole, fl_bytes = _guarded(4 * n)
    fl = fl_bytes.view(torch.int32)
    ok.fill_(7)
    fl.fill_(-1)
    eng.ecdsa_verify_dev(dq, de, ds, ok, fl)
    torch.cuda.synchronize()
    assert bool((ok_whole[-GUARD:] == 0xA5).all().item()) and bool((fl_whole[-GUARD:] == 0xA5).all().item())
    return ok.cpu().numpy(), fl.cpu().numpy().view(np.uint32)


def _mismatches(cases, ok, flags):
    return [(c["name"], c["ok"], c["flags"], int(o), int(f)) for c, o, f in zip(cases, ok, flags)
            if int(o) != int(c["ok"]) or int(f) != c["flags"]]


def verify_both(eng, cases):
    """mismatches of the host form and of the *_dev form on one batch"""
    rows = _rows(cases)
    ok, flags = eng.ecdsa_verify_wire(*rows)
    assert ok.shape == flags.shape == (len(cases),)
    ok_d, flags_d = _dev_verify(eng, *rows)
    return [("host",) + m for m in _mismatches(cases, ok, flags)] + \
           [("dev",) + m for m in _mismatches(cases, ok_d, flags_d)]


def flat(pairs):
    """[row, twin, row, twin, ...]: valid and tampered alternate"""
    return [r for pair in pairs for r in pair[:2]]


EDGE_BATCH, EDGE_ROWS = 65, (0, 63, 64)          # a 64-lane workgroup's first and last row, and the next one's


def edge_batches(special):
    """65-row batches of ordinary signatures with the special rows, three a batch, at rows 0, 63 and
    64 = n - 1: the last lane of one workgroup and the only lane of the next"""
    ordinary = C.ordinary_rows()
    for k in range(0, len(special), len(EDGE_ROWS)):
        batch = [ordinary[(i + k) % len(ordinary)] for i in range(EDGE_BATCH)]
        for pos, row in zip(EDGE_ROWS, special[k: k + len(EDGE_ROWS)]):
            batch[pos] = row
        yield batch


def test_ordinary_rows(eng):
    """the neighbours of the mixed batches, by themselves"""
    assert verify_both(eng, list(C.ordinary_rows())) == []


# ------------------------------------------------------------------ mod n: the signature's s
def test_inverter_rows_in_one_batch(eng):
    """every slow, tied and quotient s with its twin: verdict True / False, flags 0"""
    cases = flat(C.inverter_rows())
    assert len(cases) >= 2 * (3 * 8 + 3 + 8 + 2 + 4)
    assert verify_both(eng, cases) == []


def test_inverter_rows_alone(eng):
    """each as a batch of one: no neighbour's lanes beside it"""
    bad = []
    for c in flat(C.inverter_rows()):
        bad += verify_both(eng, [c])
    assert bad == []


def test_inverter_rows_at_workgroup_edges(eng):
    bad = []
    for batch in edge_batches(flat(C.inverter_rows())):
        bad += verify_both(eng, batch)
    assert bad == []


# ------------------------------------------------------------------ the ladder
def test_ladder_rows_in_one_batch(eng):
    """acc == +-addend at the G and the Q addition of windows 0, 1, 31, 62, 63: valid, flags 0 (bit 2
    clear: the sum is at infinity only mid-chain), and the twins refused"""
    cases = flat(C.ladder_rows())
    assert len(cases) == 38
    assert verify_both(eng, cases) == []
    ok, flags = eng.ecdsa_verify_wire(*_rows(cases))
    assert not (flags & 4).any() and list(ok) == [True, False] * 19


def test_ladder_rows_alone(eng):
    bad = []
    for c in flat(C.ladder_rows()):
        bad += verify_both(eng, [c])
    assert bad == []


def test_ladder_rows_among_mixed_neighbours(eng):
    bad = []
    for batch in edge_batches(flat(C.ladder_rows())):
        bad += verify_both(eng, batch)
    assert bad == []


# ------------------------------------------------------------------ mod p: hash to curve's den
def h2c(eng, ubs):
    """flm_h2c_from_uniform on the rows ubs -> (out (n, 64), flags (n,)); the GUARD_ROWS rows past n
    of both are checked here"""
    from flamingo_amd._lib import p_u8, p_u32
    n = len(ubs)
    uni = np.frombuffer(b"".join(ubs), np.uint8).reshape(n, 96).copy()
    out = np.full((n + GUARD_ROWS, 64), GUARD8, np.uint8)
    fl = np.full(n + GUARD_ROWS, GUARD32, np.uint32)
    rc = eng.lib.flm_h2c_from_uniform(eng.ctx, p_u8(uni), n, p_u8(out), p_u32(fl))
    assert rc == 0, eng.lib.flm_last_error(eng.ctx).decode()
    assert np.all(out[n:] == GUARD8) and np.all(fl[n:] == GUARD32), "wrote past row n"
    return out[:n], fl[:n]


def h2c_mismatches(eng, rows):
    out, fl = h2c(eng, [r.ub for r in rows])
    bad = []
    for i, r in enumerate(rows):
        wire, flag = C.H.expect(r.ub)
        assert flag == 0
        if out[i].tobytes() != wire or int(fl[i]) != 0:
            bad.append((i, r.name, hex(int(fl[i])), out[i].tobytes().hex()[:16], wire.hex()[:16]))
    return bad


def test_den_rows_in_one_batch(eng):
    """every solved den, in the even and in the odd lane of its pair: points byte for byte, flags 0"""
    rows = C.den_rows()
    assert {r.lane for r in rows} == {0, 1}
    assert h2c_mismatches(eng, rows) == []


def test_den_rows_alone(eng):
    bad = []
    for r in C.den_rows():
        bad += h2c_mismatches(eng, [r])
    assert bad == []


def test_den_rows_at_workgroup_edges(eng):
    """34-row batches (a 64-lane workgroup holds 32 rows) with den rows at rows 0, 31, 32 and 33 = n - 1,
    ordinary rows elsewhere"""
    special, at, bad = C.den_rows(), (0, 31, 32, 33), []
    for k in range(0, len(special), len(at)):
        batch = [C.den_ordinary(i) for i in range(34)]
        for pos, row in zip(at, special[k: k + len(at)]):
            batch[pos] = row
        bad += h2c_mismatches(eng, batch)
    assert bad == []
