"""encode_gauss_mask_kernel bit for bit against the numpy restatement of the table-sampled noise
(tests/dgauss_cases.py): one batch of four clients with 0, 1, 5 and 14 seeds at every width, real and crafted tables,
three lengths and both roundings, host and device forms with poisoned padding and guards, clipped counts included;
whole rounds through the existing noise-aware decodes at noise_bits = 2 tau, also through the store; the refusals; and
the device form's promise that a table it cannot check keeps every field inside its headroom."""
from __future__ import annotations

import ctypes
import functools
import hashlib
import importlib.util
import os

import numpy as np
import pytest

import codec_cases as K
import dgauss_cases as G
import dp_cases as D
import pack_cases as PC

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POISON = 0xDEADBEEF
N = len(D.BATCH_SEEDS)


@pytest.fixture(scope="module")
def eng():
    from flamingo_amd import MaskEngine
    e = MaskEngine(0)
    yield e
    e.close()


def _u8(seeds32):
    return np.frombuffer(b"".join(seeds32), np.uint8).reshape(len(seeds32), 32).copy()


def _tag(name: str) -> int:
    return 300 + sorted(TABLES).index(name)


def _decisive_high_word(tag: int) -> int:
    """The high word of a draw of client 0 of the batch `tag` whose low word lies in [2^31, 8/9 2^32): against
    low_word_table(that word) the parameter's count is decided by the low word alone, is 4 or more of 8, and a signed
    compare of the low half would make it 0.  The draws of a parameter do not depend on L."""
    u = G.draws_u64(D.seed(100 * tag + 0), 17)
    lo = u & np.uint64(0xFFFFFFFF)
    pick = np.flatnonzero((lo >= np.uint64(2 ** 31)) & (lo < np.uint64(8 * 2 ** 32 // 9)))
    assert len(pick), "no draw of the first 17 with such a low word: choose another tag"
    return int(u[pick[0]] >> np.uint64(32))


TABLES = {
    "gauss 0.5,5": lambda: G.real_table(0.5, 5),
    "gauss 3.2,32": lambda: G.real_table(3.2, 32),
    "gauss 51.2,512": lambda: G.real_table(51.2, 512),
    "all zeros": lambda: G.all_zeros(3),
    "all ones": lambda: G.all_ones(3),
    "coin": G.coin,
    "even steps, T = 74": G.even_steps,
    "low word only": lambda: G.low_word_table(_decisive_high_word(_tag("low word only"))),
    "across bit 63": G.top_bit_table,
}


@functools.lru_cache(maxsize=None)
def _table(name: str) -> np.ndarray:
    t = TABLES[name]()
    t.setflags(write=False)
    return t


def _cases():
    taus = {"gauss 0.5,5": 5, "gauss 3.2,32": 32, "gauss 51.2,512": 512, "all zeros": 3, "all ones": 3, "coin": 1,
            "even steps, T = 74": G.ODD_TAU, "low word only": 4, "across bit 63": 4}
    return [(name, P, f, c) for name in TABLES for P, f, c in G.gpu_params(taus[name])]


@functools.lru_cache(maxsize=None)
def _batch(L: int, c: float, tag: int):
    return D.batch(L, c, tag)


def _check_table_premise(name, cdt, noises, L):
    """What a crafted table is there to show, asserted on the restatement itself."""
    z = np.stack([G.counts(s, L, cdt) for s in noises])
    T = len(cdt)
    if name == "all zeros":
        assert np.all(z == T)
    elif name == "all ones":
        assert np.all(z == 0)
    elif name == "coin":
        assert set(np.unique(z)) == {0, 2}
    elif name.startswith("even steps") and L == 2077:
        assert all(set(row) == set(range(T + 1)) for row in z)             # every count 0..74, in every client's row
    elif name == "low word only":
        hi = int(cdt[0]) >> 32
        u = G.draws_u64(noises[0], L)
        decided = np.flatnonzero((u >> np.uint64(32)) == np.uint64(hi))
        assert len(decided) and all(4 <= z[0, l] < T for l in decided)      # the low word alone decides, and not at an end
    elif name == "across bit 63":
        u = G.draws_u64(noises[0], L)
        assert (u < np.uint64(2 ** 63)).any() and (z[0] == 0).any() and (z[0] > 0).any()


# ------------------------------------------------------------------ one batch, every case
@pytest.mark.parametrize("name,P,f,c", _cases())
def test_batch_matches_the_restatement(eng, name, P, f, c):
    import torch
    cdt = _table(name)
    tag = _tag(name)
    ct = torch.from_numpy(cdt.view(np.int64).copy()).cuda()
    for L in G.LENGTHS:
        Lw = -(-L // P)
        xs, seg, seeds, signs, dithers, noises = _batch(L, c, tag)
        _check_table_premise(name, cdt, noises, L)
        sd, nz, di = torch.from_numpy(seeds).cuda(), torch.from_numpy(_u8(noises)).cuda(), torch.from_numpy(_u8(dithers)).cuda()
        XP, OP = (L + 3) // 4 * 4 + 16, (Lw + 3) // 4 * 4 + 32
        xp = np.full((N, XP), np.nan, np.float32)                               # x rows longer than L with NaN behind them
        xp[:, :L] = xs
        xt = torch.from_numpy(xp).cuda()
        for d, dd in ((None, None), (dithers, di)):
            want, want_cl = G.batch_rows(xs, seg, seeds, signs, f, c, P, d, noises, cdt)
            if P == 1:                                                          # the counts of the call without noise
                _, plain_cl = eng.client_encode_mask(seg, seeds, signs, L, xs, f, c, dither=d, return_clipped=True)
            else:
                _, plain_cl = eng.client_encode_pack_mask(seg, seeds, signs, L, xs, f, c, P, dither=d, return_clipped=True)
            assert plain_cl.sum() > 0 and np.array_equal(want_cl, plain_cl)
            got, cl = eng.client_encode_gauss_mask(seg, seeds, signs, L, xs, f, c, cdt, noises, pack=P, dither=d,
                                                   return_clipped=True)
            assert got.shape == (N, Lw) and np.array_equal(got, want), (L, "stochastic" if d else "nearest")
            assert np.array_equal(cl, want_cl), L
            out = torch.full((N, OP), POISON - (1 << 32), dtype=torch.int32, device="cuda")   # guard words behind each row
            clt = torch.full((N,), 77, dtype=torch.int32, device="cuda")
            eng.client_encode_gauss_mask_dev(seg, sd, signs, out, L, xt, f, c, ct, nz, pack=P, dither_dev=dd, clipped=clt)
            o = out.cpu().numpy().view(np.uint32)
            assert np.array_equal(o[:, :Lw], want), (L, "device")
            assert np.all(o[:, Lw:] == POISON)
            assert np.array_equal(clt.cpu().numpy().view(np.uint32), want_cl)


# ------------------------------------------------------------------ whole rounds through the existing decodes
ROUNDS = ((2, 1.0, 4, 5, 14, 2077), (2, 1.0, 4, 5, 1, 2077), (7, 1.0, 2, 512, 51, 1025), (7, 1.0, 2, 512, 1, 1025),
          (16, 4.0, 1, 32, 3, 1025))                                           # (f, c, P, tau, n, L)


@pytest.mark.parametrize("f,c,P,tau,n,L", ROUNDS)
def test_rows_decode_with_the_noise_decodes_at_twice_the_tail(eng, f, c, P, tau, n, L):
    """n clients (at P > 1 the most the headroom admits, or one), every third at +c everywhere, mixed roundings, each
    under a self mask the server removes.  The unmasked sum is the sum of the restatement's noised encodings; decoded
    with the binomial noise's decode calls at noise_bits = 2 tau (flm_decode_sum unpacked) it is the restatement's
    decode byte for byte, on the engine and through the store."""
    import torch
    from flamingo_amd.ingest import VectorStore
    assert G.headroom_ok(f, c, P, tau, n) and (P == 1 or n == 1 or not G.headroom_ok(f, c, P, tau, n + 1))
    cdt = G.real_table(tau / 10.0, tau)
    xs, dithers = PC.worst_inputs(f, c, n, L)
    own = [hashlib.sha256(b"dgauss self %d" % i).digest() for i in range(n)]
    zs = [D.seed(700 + i) for i in range(n)]
    rows = {}
    for stochastic in (False, True):                         # a call rounds all its clients one way: two calls
        ids = [i for i in range(n) if (dithers[i] is not None) == stochastic]
        if not ids:
            continue
        seg = np.arange(len(ids) + 1, dtype=np.int64)
        y = eng.client_encode_gauss_mask(seg, [own[i] for i in ids], [1] * len(ids), L, np.stack([xs[i] for i in ids]), f, c,
                                         cdt, [zs[i] for i in ids], pack=P,
                                         dither=[dithers[i] for i in ids] if stochastic else None)
        rows.update(zip(ids, y))
    rows = np.stack([rows[i] for i in range(n)])
    total = eng.aggregate_unmask(rows, own, [-1] * n)
    enc = sum(G.encode_any(xs[i], f, c, P, cdt, zs[i], dithers[i])[0].astype(np.uint64) for i in range(n))
    assert np.array_equal(total, (enc & 0xFFFFFFFF).astype(np.uint32))
    want = G.decode_any(total, L, f, c, P, tau, n)
    if P == 1:
        assert eng.decode_sum(total, f, n).tobytes() == want.tobytes()
        return
    Lw = -(-L // P)
    tt = torch.zeros((Lw + 3) // 4 * 4, dtype=torch.int32, device="cuda")
    tt[:Lw] = torch.from_numpy(total.view(np.int32).copy()).cuda()
    ot = torch.zeros((L + 3) // 4 * 4, dtype=torch.float32, device="cuda")
    eng.decode_unpack_dev(tt, ot, L, f, c, P, n, noise_bits=2 * tau)
    assert ot.cpu().numpy()[:L].tobytes() == want.tobytes()
    assert eng.decode_unpack(total, L, f, c, P, n, noise_bits=2 * tau).tobytes() == want.tobytes()
    st = VectorStore(eng, Lw, n)
    for i in range(n):
        st.add(i, rows[i])
    st.partial_sum()
    st.wait_partial()
    assert st.unmask_unpack_f32(own, [-1] * n, L, f, c, P, n, noise_bits=2 * tau).tobytes() == want.tobytes()
    if n > 1:
        with pytest.raises(RuntimeError):                    # one contributor more has no headroom at this tail
            st.unmask_unpack_f32(own, [-1] * n, L, f, c, P, n + 1, noise_bits=2 * tau)
    st.close()


# ------------------------------------------------------------------ refusals
def test_refusals_launch_nothing(eng):
    import torch
    from flamingo_amd._lib import p_f32, p_i64, p_i8, p_u8, p_u32, p_u64
    seg = np.array([0, 1], np.int64)
    seeds, signs = _u8([D.seed(1)]), np.array([1], np.int8)
    noise = _u8([D.seed(2)])
    x = np.zeros((1, 8), np.float32)
    out = np.full(8, POISON, np.uint32)
    cl = np.full(1, 77, np.uint32)
    good = G.real_table(0.5, 5)
    down = good.copy()
    down[7] = down[6] - np.uint64(1)
    enc = eng.lib.flm_client_encode_gauss_mask
    err = lambda: eng.lib.flm_last_error(eng.ctx)   # noqa: E731

    def call(f, c, P, tau, table, nz):
        return enc(eng.ctx, p_f32(x), 1, p_i64(seg), p_u8(seeds), p_i8(signs), 8, f, c, P, None, tau,
                   p_u64(table) if table is not None else None, nz, p_u32(out), p_u32(cl))

    assert call(4, 1.0, 2, 5, good, None) == -1 and b"noise seeds" in err()
    assert call(4, 1.0, 2, 5, None, p_u8(noise)) == -1 and b"NULL" in err()
    for tau in (0, 513, -3):                                                     # tail = 0 is not "off"
        assert call(4, 1.0, 2, tau, good, p_u8(noise)) == -1 and err() == b"tail must be in 1..512", tau
    assert call(4, 1.0, 2, 5, down, p_u8(noise)) == -1 and err() == b"the table must be non-decreasing"
    assert call(4, 1.0, 3, 5, good, p_u8(noise)) == -1 and b"pack" in err()
    assert call(2, 1.0, 4, 124, G.all_zeros(124), p_u8(noise)) == -4 and b"headroom" in err()   # one client has no room
    assert call(7, 1.0, 4, 1, G.coin(), p_u8(noise)) == -4
    assert np.all(out == POISON) and cl[0] == 77
    assert call(4, 1.0, 2, 5, good, p_u8(noise)) == 0 and not np.all(out == POISON)
    # the device form: a misaligned table pointer, refused by code and text before anything is launched or staged
    xt = torch.zeros((1, 8), dtype=torch.float32, device="cuda")
    ot = torch.full((1, 8), 5, dtype=torch.int32, device="cuda")
    sd, nz = torch.from_numpy(seeds).cuda(), torch.from_numpy(noise).cuda()
    ct = torch.from_numpy(np.concatenate([good, good[:1]]).view(np.int64).copy()).cuda()
    dev = eng.lib.flm_client_encode_gauss_mask_dev
    vp = ctypes.c_void_p

    def call_dev(table_ptr, noise_ptr):
        return dev(eng.ctx, vp(xt.data_ptr()), 8, 1, p_i64(seg), vp(sd.data_ptr()), p_i8(signs), 8, 4, 1.0, 2, None, 5,
                   vp(table_ptr), vp(noise_ptr), vp(ot.data_ptr()), 8, None, None)

    assert call_dev(ct.data_ptr() + 4, nz.data_ptr()) == -1 and err() == b"cdt must be 8-byte aligned"
    assert call_dev(0, nz.data_ptr()) == -1 and call_dev(ct.data_ptr(), 0) == -1
    torch.cuda.synchronize()
    assert np.all(ot.cpu().numpy() == 5)
    assert call_dev(ct.data_ptr() + 8, nz.data_ptr()) == 0                       # 8-byte aligned is enough
    torch.cuda.synchronize()
    assert not np.all(ot.cpu().numpy() == 5)
    eng.codec_check_gauss(4, 1.0, 15, 1057, pack=2, L=2077)
    with pytest.raises(RuntimeError, match="code -4"):
        eng.codec_check_gauss(4, 1.0, 15, 1058, pack=2)
    with pytest.raises(RuntimeError, match="code -1"):
        eng.codec_check_gauss(4, 1.0, 0, 1, pack=2)


# ------------------------------------------------------------------ the device form's in-range promise
@pytest.mark.parametrize("P,f,c", ((1, 7, 1.0), (2, 7, 1.0), (4, 2, 1.0)))
def test_device_form_keeps_fields_in_range_whatever_the_table_holds(eng, P, f, c):
    """The device form cannot see its table.  Handed one with decreases (a real table reversed, and pseudo-random
    entries) it returns 0 and, on the unmasked call (a client with no seeds), every field stays within [0, 2 B_n]:
    the count is in [0, T] whatever the entries are.  Not a fault test: every probe reads inside the table."""
    import torch
    tau, L = 37, 2077
    Lw = -(-L // P)
    bn = G.bias_n(f, c, tau)
    x = K.random_row(L, c, 5, wild=True)[None, :]
    xt = torch.from_numpy(np.ascontiguousarray(np.pad(x, ((0, 0), (0, 3))))).cuda()
    seg = np.zeros(2, np.int64)
    sd = torch.zeros((0, 32), dtype=torch.uint8, device="cuda")
    nz = torch.from_numpy(_u8([D.seed(41)])).cuda()
    rng = np.random.default_rng(37)
    for bad in (G.even_steps(tau)[::-1].copy(), rng.integers(0, 2 ** 64, 2 * tau, dtype=np.uint64)):
        assert np.any(bad[1:] < bad[:-1])
        out = torch.zeros((1, (Lw + 3) // 4 * 4), dtype=torch.int32, device="cuda")
        eng.client_encode_gauss_mask_dev(seg, sd, np.zeros(0, np.int8), out, L, xt, f, c,
                                         torch.from_numpy(bad.view(np.int64).copy()).cuda(), nz, pack=P)
        o = out.cpu().numpy().view(np.uint32)[0, :Lw]
        if P == 1:
            q = o.view(np.int32).astype(np.int64) + bn                            # the word is q', the field q' + B_n
        else:
            W = 32 // P
            q = ((o.astype(np.int64)[:, None] >> (W * np.arange(P, dtype=np.int64))) & (2 ** W - 1)).reshape(-1)[:L]
        assert q.min() >= 0 and q.max() <= 2 * bn
        plain = K.encode(x[0], f, c)[0].view(np.int32).astype(np.int64)          # and the count itself is in [0, T]
        count = q - PC.bias(f, c) - plain
        assert count.min() >= 0 and count.max() <= 2 * tau


# ------------------------------------------------------------------ the reference-side binding
def test_reference_side_binding(eng, monkeypatch):
    """integration/util_flm.py's call, once per width, against the restatement."""
    monkeypatch.setenv("FLM_LIB", os.path.join(ROOT, "flamingo_amd", "lib", "libflamingo_hip.so"))
    import torch  # noqa: F401  (one HIP runtime per process: torch's, loaded first)
    spec = importlib.util.spec_from_file_location("util_flm", os.path.join(ROOT, "integration", "util_flm.py"))
    flm = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(flm)
    f, c, P, tau, L = 4, 1.0, 2, 15, 1027
    cdt = G.real_table(1.5, tau)
    xs, seg, seeds, signs, dithers, noises = D.batch(L, c, 3)
    flm.codec_check_gauss(f, c, P, tau, 1057, L)
    with pytest.raises(RuntimeError):
        flm.codec_check_gauss(f, c, P, tau, 1058)
    k0, k1 = int(seg[3]), int(seg[4])
    sd, sg = [bytes(s) for s in seeds[k0:k1]], list(signs[k0:k1])
    for pack in (1, P):
        want, want_cl = G.masked(xs[3], f, c, pack, seeds[k0:k1], signs[k0:k1], cdt, noises[3], dithers[3])
        got, cl = flm.client_encode_gauss_mask(sd, sg, L, xs[3], f, c, cdt, noises[3], pack=pack, dither=dithers[3])
        assert np.array_equal(got, want) and cl == want_cl
