"""flm_feldman_verify on the GPU against both fixtures -- the reference's own verdicts
(tests/golden/dkg_golden.json) and the edge cases of tests/feldman_cases.py -- on verdict, flags and
points_out, through the host-pointer call and the *_dev call; batches around the wave size in the
grid form and with a permuted dealer array; the argument errors; the *_dev call's stream contract;
and the round trip deal -> commit -> check -> interpolate -> group key through the C ABI."""
from __future__ import annotations

import ctypes
import functools
import importlib.util
import os

import numpy as np
import pytest

import ec_oracle as E
import feldman_cases as F

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 64
N = E.N


def _generator():
    spec = importlib.util.spec_from_file_location("make_dkg_golden",
                                                  os.path.join(ROOT, "tests", "golden", "make_dkg_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


G = _generator()


@pytest.fixture(scope="module")
def eng():
    from flamingo_amd import MaskEngine
    e = MaskEngine(0)
    yield e
    e.close()


# ------------------------------------------------------------------ rows and their expectations
def _arrays(rows):
    """rows [(com [T] of 64 bytes, x, share int)] with one T -> the row form's arrays: every row its own
    dealer (M = n): commitments (T, n, 64), dealer (n,), xs (n,), shares (n, 32)."""
    n, T = len(rows), len(rows[0][0])
    com = np.zeros((T, n, 64), np.uint8)
    for i, (c, _, _) in enumerate(rows):
        for k in range(T):
            com[k, i] = np.frombuffer(c[k], np.uint8)
    xs = np.array([x for _, x, _ in rows], np.uint32)
    sh = np.frombuffer(b"".join(int(s).to_bytes(32, "big") for _, _, s in rows), np.uint8).reshape(n, 32).copy()
    return com, np.arange(n, dtype=np.uint32), xs, sh


def _want(results):
    ok = np.array([r[0] for r in results], bool)
    fl = np.array([r[1] for r in results], np.uint32)
    pts = np.frombuffer(b"".join(r[2] for r in results), np.uint8).reshape(-1, 64)
    return ok, fl, pts


def _guarded(nbytes):
    """A device byte buffer of nbytes followed by GUARD bytes of 0xA5 -> (whole, payload view)."""
    import torch
    whole = torch.full((nbytes + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    return whole, whole[:nbytes]


def _guard_intact(whole):
    return bool((whole[-GUARD:] == 0xA5).all().item())


def _dev_verify(eng, com, dealer, xs, sh, x_bits, points=True, flags=True):
    """the *_dev call on guarded outputs -> (ok, flags or None, points or None); guards checked here"""
    import torch
    n = sh.shape[0]
    dc, ds = torch.from_numpy(com).cuda(), torch.from_numpy(sh).cuda()
    dx = torch.from_numpy(xs.view(np.int32)).cuda()
    dd = torch.from_numpy(dealer.view(np.int32)).cuda() if dealer is not None else None
    ok_whole, ok = _guarded(n)
    fl_whole, fl_bytes = _guarded(4 * n)
    pt_whole, pt_bytes = _guarded(64 * n)
    fl, pt = fl_bytes.view(torch.int32), pt_bytes.view(n, 64)
    ok.fill_(7)
    fl.fill_(-1)
    pt.fill_(0x5C)
    eng.feldman_verify_dev(dc, dd, dx, ds, x_bits, ok, pt if points else None, fl if flags else None)
    torch.cuda.synchronize()
    assert _guard_intact(ok_whole) and _guard_intact(fl_whole) and _guard_intact(pt_whole)
    if not flags:
        assert bool((fl == -1).all().item()), "a NULL flags pointer must leave memory alone"
    if not points:
        assert bool((pt == 0x5C).all().item()), "a NULL points pointer must leave memory alone"
    return (ok.cpu().numpy(), fl.cpu().numpy().view(np.uint32) if flags else None,
            pt.cpu().numpy() if points else None)


def _check(got, want, labels):
    ok, fl, pts = got
    wok, wfl, wpts = want
    bad = [(labels[i], bool(ok[i]), int(fl[i]), bool(wok[i]), int(wfl[i])) for i in range(len(labels))
           if bool(ok[i]) != bool(wok[i]) or int(fl[i]) != int(wfl[i])]
    assert bad == []
    wrong = [labels[i] for i in range(len(labels)) if bytes(pts[i]) != bytes(wpts[i])]
    assert wrong == []


# ------------------------------------------------------------------ the edge cases
@pytest.mark.parametrize("shape", sorted(F.groups()), ids=lambda s: f"T{s[0]}_bits{s[1]}")
def test_edge_cases_host_and_dev(eng, shape):
    cases = F.groups()[shape]
    rows = [(c.com, c.x, c.share) for c in cases]
    want = _want([F.expected(c.com, c.x, c.x_bits, c.share) for c in cases])
    assert [bool(v) for v in want[0]] == [c.ok for c in cases] and [int(v) for v in want[1]] == [c.flags for c in cases]
    com, dealer, xs, sh = _arrays(rows)
    labels = [c.name for c in cases]
    got = eng.feldman_verify_wire(com, dealer, xs, sh, x_bits=shape[1], points=True)
    assert got[0].dtype == bool and got[1].dtype == np.uint32
    _check(got, want, labels)
    _check(_dev_verify(eng, com, dealer, xs, sh, shape[1]), want, labels)


def test_edge_cases_alone(eng):
    """each case as a batch of one: no neighbour's lanes beside it, the wave diverges nowhere"""
    for c in F.CASES:
        com, dealer, xs, sh = _arrays([(c.com, c.x, c.share)])
        got = eng.feldman_verify_wire(com, None, xs, sh, x_bits=c.x_bits, points=True)
        _check(got, _want([F.expected(c.com, c.x, c.x_bits, c.share)]), [c.name])


# ------------------------------------------------------------------ the reference's verdicts
@functools.lru_cache(maxsize=None)
def _reference_rows():
    out = {}
    for n, T, com, x, share, ok, label in G.rows(G.load()):
        out.setdefault(n, []).append((tuple(com), x, int.from_bytes(share, "big"), ok, label))
    return out


@pytest.mark.parametrize("n", [6, 60])
def test_reference_verdicts_host_and_dev(eng, n):
    recs = _reference_rows()[n]
    rows = [r[:3] for r in recs]
    bits = n.bit_length()
    want = _want([F.expected(c, x, bits, s) for c, x, s in rows])
    assert [bool(v) for v in want[0]] == [r[3] for r in recs], "the oracle and the reference disagree"
    com, dealer, xs, sh = _arrays(rows)
    labels = [r[4] for r in recs]
    _check(eng.feldman_verify_wire(com, dealer, xs, sh, x_bits=bits, points=True), want, labels)
    _check(_dev_verify(eng, com, dealer, xs, sh, bits), want, labels)


def test_reference_grid_form(eng):
    """the n = 6 honest grid as the members see it: NULL dealer, row i = dealer i % 6 at x = i // 6 + 1"""
    fx = G.load()["groups"][0]
    assert fx["n"] == 6
    com = np.zeros((fx["T"], 6, 64), np.uint8)
    for d in range(6):
        for k, h in enumerate(fx["commitments"][str(d + 1)]):
            com[k, d] = np.frombuffer(bytes.fromhex(h), np.uint8)
    honest = {(r["dealer"], r["x"]): bytes.fromhex(r["share"]) for r in fx["records"] if r["kind"] == "honest"}
    sh = np.frombuffer(b"".join(honest[(i % 6 + 1, i // 6 + 1)] for i in range(36)), np.uint8).reshape(36, 32)
    xs = np.array([i // 6 + 1 for i in range(36)], np.uint32)
    ok, fl, pts = eng.feldman_verify_wire(com, None, xs, sh, points=True)
    assert ok.all() and not fl.any()
    # F_d(x) is the share's public point
    assert [bytes(p) for p in pts] == [E.wire(E.mul(int.from_bytes(bytes(s), "big"))) for s in sh]
    ok2, _, _ = eng.feldman_verify_wire(com, None, xs, np.roll(sh, 1, axis=0))
    assert not ok2.any()


# ------------------------------------------------------------------ batch edges
@pytest.mark.parametrize("n", [1, 63, 64, 65, 129])
def test_batch_edges_row_form_and_permuted_dealers(eng, n):
    rows_all, res_all = F.pool()
    idx = [(i + 2 * (i // 32)) % len(rows_all) for i in range(n)]       # valid and invalid alternate in every wave
    rows, want = [rows_all[i] for i in idx], _want([res_all[i] for i in idx])
    com, dealer, xs, sh = _arrays(rows)
    labels = [f"row{i}" for i in range(n)]
    got = eng.feldman_verify_wire(com, dealer, xs, sh, x_bits=32, points=True)
    _check(got, want, labels)
    if n > 1:
        assert 0 < int(got[0].sum()) < n
    _check(_dev_verify(eng, com, dealer, xs, sh, 32), want, labels)
    # points_out = NULL changes nothing else
    ok0, fl0, none = eng.feldman_verify_wire(com, dealer, xs, sh, x_bits=32, points=False)
    assert none is None and (ok0 == got[0]).all() and (fl0 == got[1]).all()
    ok1, fl1, none = _dev_verify(eng, com, dealer, xs, sh, 32, points=False)
    assert none is None and (ok1.astype(bool) == got[0]).all() and (fl1 == got[1]).all()
    # every share against the next row's commitments: a permuted dealer array
    perm = (np.arange(n, dtype=np.uint32) + 1) % n
    want_p = _want([F.expected(rows[int(perm[i])][0], rows[i][1], 32, rows[i][2]) for i in range(n)])
    _check(eng.feldman_verify_wire(com, perm, xs, sh, x_bits=32, points=True), want_p, labels)
    _check(_dev_verify(eng, com, perm, xs, sh, 32), want_p, labels)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 129])
def test_batch_edges_grid_form(eng, n):
    """NULL dealer: row i belongs to dealer i % M.  M = 5 dealers of the pool, so consecutive lanes
    read different columns and a wave's lanes hold different x."""
    rows_all, _ = F.pool()
    M = 5
    dealers = [rows_all[2 * d][0] for d in range(M)]
    com = np.zeros((F.POOL_T, M, 64), np.uint8)
    for d in range(M):
        for k in range(F.POOL_T):
            com[k, d] = np.frombuffer(dealers[d][k], np.uint8)
    rows = [(dealers[i % M], rows_all[(3 * i) % len(rows_all)][1], rows_all[2 * (i % M)][2]) for i in range(n)]
    want = _want([F.expected(c, x, 32, s) for c, x, s in rows])
    xs = np.array([r[1] for r in rows], np.uint32)
    sh = np.frombuffer(b"".join(int(r[2]).to_bytes(32, "big") for r in rows), np.uint8).reshape(n, 32).copy()
    labels = [f"row{i}" for i in range(n)]
    _check(eng.feldman_verify_wire(com, None, xs, sh, x_bits=32, points=True), want, labels)
    _check(_dev_verify(eng, com, None, xs, sh, 32), want, labels)
    explicit = np.arange(n, dtype=np.uint32) % M
    _check(eng.feldman_verify_wire(com, explicit, xs, sh, x_bits=32, points=True), want, labels)


# ------------------------------------------------------------------ arguments
def test_argument_errors_write_nothing(eng):
    import torch
    FLM_EINVAL = -1                   # include/flamingo_hip.h
    lib, ctx = eng.lib, eng.ctx
    c = F.BY_NAME["share_1"]
    com, dealer, xs, sh = _arrays([(c.com, c.x, c.share)] * 4)
    T, M, n = com.shape[0], com.shape[1], 4
    from flamingo_amd._lib import p_u8, p_u32
    ok = np.full(n, 7, np.uint8)
    fl = np.full(n, 0xFFFFFFFF, np.uint32)
    pts = np.full((n, 64), 0x5C, np.uint8)

    def host(T=T, M=M, dealer=dealer, xs=xs, bits=6, sh=sh, n=n, com=com, ok=ok):
        return lib.flm_feldman_verify(ctx, p_u8(com) if com is not None else None, T, M,
                                      p_u32(dealer) if dealer is not None else None,
                                      p_u32(xs) if xs is not None else None, bits,
                                      p_u8(sh) if sh is not None else None, n,
                                      p_u8(ok) if ok is not None else None, p_u8(pts), p_u32(fl))
    bad_dealer = dealer.copy()
    bad_dealer[2] = M
    for kw in (dict(T=0), dict(M=0), dict(T=-1), dict(bits=0), dict(bits=33), dict(n=-1), dict(n=(1 << 26) + 1),
               dict(com=None), dict(xs=None), dict(sh=None), dict(ok=None), dict(dealer=bad_dealer)):
        assert host(**kw) == FLM_EINVAL, kw
        assert (ok == 7).all() and (fl == 0xFFFFFFFF).all() and (pts == 0x5C).all(), kw
    assert b"dealer[2] = 4" in lib.flm_last_error(ctx)       # the last refusal: the host form checks dealer < M
    assert host(n=0) == 0 and (ok == 7).all() and (fl == 0xFFFFFFFF).all() and (pts == 0x5C).all()
    assert lib.flm_feldman_verify(ctx, None, 1, 1, None, None, 1, None, 0, None, None, None) == 0
    assert host() == 0 and ok.all() and not fl.any()

    vp = ctypes.c_void_p
    z = lambda *s: torch.zeros(s, dtype=torch.uint8, device="cuda")  # noqa: E731
    dok = torch.full((n,), 7, dtype=torch.uint8, device="cuda")
    dc, ds, dx = z(T, M, 64), z(n, 32), torch.zeros(n, dtype=torch.int32, device="cuda")

    def dev(T=T, M=M, bits=6, n=n, com=dc, xs=dx, sh=ds, ok=dok):
        p = lambda t: vp(t.data_ptr()) if t is not None else vp()  # noqa: E731
        return lib.flm_feldman_verify_dev(ctx, p(com), T, M, vp(), p(xs), bits, p(sh), n, p(ok), vp(), vp(), vp())
    for kw in (dict(T=0), dict(M=0), dict(bits=0), dict(bits=33), dict(n=-1), dict(n=(1 << 26) + 1),
               dict(com=None), dict(xs=None), dict(sh=None), dict(ok=None)):
        assert dev(**kw) == FLM_EINVAL, kw
    assert dev(n=0) == 0
    torch.cuda.synchronize()
    assert bool((dok == 7).all().item())
    q = z(64 * T * M + 16)
    with pytest.raises(RuntimeError, match="16-byte aligned"):
        eng.feldman_verify_dev(q[1:1 + 64 * T * M].view(T, M, 64), None, dx, ds, 6, dok)
    with pytest.raises(RuntimeError, match="4 shares for 3 evaluation points"):
        eng.feldman_verify_wire(com, None, xs[:3], sh)
    with pytest.raises(RuntimeError, match="must be"):
        eng.feldman_verify_wire(com[:, :, :63], None, xs, sh)
    torch.cuda.synchronize()
    assert bool((dok == 7).all().item())


# ------------------------------------------------------------------ the *_dev form's stream contract
def _long_kernel(n=8192, reps=12):
    """Tens of ms of matmuls on the current stream (tests/test_streams_gpu.py) and their event."""
    import torch
    a = torch.ones((n, n), device="cuda")
    for _ in range(reps):
        a = a @ a * 1e-4
    ev = torch.cuda.Event()
    ev.record()
    return a, ev


def test_dev_form_does_not_block(eng):
    import torch
    rows_all, res_all = F.pool()
    rows = [rows_all[i % len(rows_all)] for i in range(65)]
    com, dealer, xs, sh = _arrays(rows)
    dc, ds = torch.from_numpy(com).cuda(), torch.from_numpy(sh).cuda()
    dx, dd = torch.from_numpy(xs.view(np.int32)).cuda(), torch.from_numpy(dealer.view(np.int32)).cuda()
    ok = torch.zeros(65, dtype=torch.uint8, device="cuda")
    eng.feldman_verify_dev(dc, dd, dx, ds, 32, ok)             # warm: the code object is loaded
    torch.cuda.synchronize()
    ok.zero_()
    _, busy = _long_kernel()
    eng.feldman_verify_dev(dc, dd, dx, ds, 32, ok)
    assert not busy.query(), "flm_feldman_verify_dev waited for earlier work on its stream"
    torch.cuda.synchronize()
    assert [bool(o) for o in ok.cpu().numpy()] == [res_all[i % len(rows_all)][0] for i in range(65)]


# ------------------------------------------------------------------ the engine's integer form
def test_engine_integer_form_matches_the_host_twin(eng):
    from flamingo_amd import crypto as C
    co = [[(7 * d + 3 * k + 1) * 0x1234567 % N for d in range(3)] for k in range(3)]          # [k][d]
    co[1][2] = 0                                                                          # an infinity commitment
    com = [[C.mul(c) if c else None for c in row] for row in co]
    xs = [1, 2, 3, 1, 2, 3]
    f = lambda d, x: sum(co[k][d] * x ** k for k in range(3)) % N  # noqa: E731
    shares = [f(i % 3, xs[i]) for i in range(6)]
    shares[4] = (shares[4] + 1) % N
    shares[5] = 1 << 256                                  # no wire form: refused
    ok, pts = eng.feldman_verify(com, None, xs, shares, points=True)
    assert ok == [True, True, True, True, False, False]
    assert ok == [C.feldman_verify(shares[i], xs[i], [com[k][i % 3] for k in range(3)]) for i in range(6)]
    assert pts == [C.feldman_point(xs[i], [com[k][i % 3] for k in range(3)]) for i in range(6)]
    assert eng.feldman_verify(com, [2, 1, 0, 0, 1, 2], xs, shares) == \
        [C.feldman_verify(shares[i], xs[i], [com[k][d] for k in range(3)]) for i, d in enumerate([2, 1, 0, 0, 1, 2])]


# ------------------------------------------------------------------ the ABI round trip
def test_abi_round_trip_deal_commit_check_interpolate(eng):
    """M = 5 dealers, T = 3 coefficients, C = 5 points: flm_shamir_deal, commitments by flm_ec_mul, the
    25-row grid all ok; the summed shares interpolate to the sum of the secrets, and that key times G is
    the sum of the C_{i,0} by flm_ec_combine."""
    import hashlib
    from flamingo_amd.abides.flamingo import seeds
    M, T, C = 5, 3, 5
    co = np.frombuffer(b"".join(hashlib.sha256(f"abi-round-trip:{i}".encode()).digest() for i in range(T * M)),
                       np.uint8).reshape(T, M, 32).copy()
    co[0, 0, 0] = 0xFF                                    # one secret above n: dealt and committed reduced
    co[0, 0, 1:5] = 0xFF
    xs = np.arange(1, C + 1, dtype=np.uint32)
    shares = eng.shamir_deal_wire(co, xs)                                     # (C, M, 32), point-major
    g = np.frombuffer(E.wire(E.G), np.uint8)
    com, flags = eng.ec_mul_wire(np.tile(g, (T * M, 1)), co.reshape(T * M, 32))
    assert not (flags & ~np.uint32(4)).any()
    com = com.reshape(T, M, 64)
    ok, fl, pts = eng.feldman_verify_wire(com, None, np.repeat(xs, M), shares.reshape(C * M, 32), points=True)
    assert ok.all() and not fl.any()
    ints = lambda a: [int.from_bytes(bytes(r), "big") for r in a]  # noqa: E731
    secrets = [v % N for v in ints(co[0])]
    sk_shares = [sum(ints(shares[c])) % N for c in range(C)]
    lam = seeds.lagrange_at_zero([int(x) for x in xs[:T]])
    key = sum(l * s for l, s in zip(lam, sk_shares[:T])) % N
    assert key == sum(secrets) % N
    lam_w = np.frombuffer(b"".join((1).to_bytes(32, "big") for _ in range(M)), np.uint8).reshape(M, 32)
    group, _, gfl = eng.ec_combine_wire(None, com[0].reshape(M, 1, 64), lam_w, negate=False)
    assert not gfl.any() and bytes(group[0]) == E.wire(E.mul(key))
    # a member's verification key: the sum over dealers of F_d(x) is its share's public point
    vk, _, _ = eng.ec_combine_wire(None, pts.reshape(C, M, 64)[0].reshape(M, 1, 64), lam_w, negate=False)
    assert bytes(vk[0]) == E.wire(E.mul(sk_shares[0]))
