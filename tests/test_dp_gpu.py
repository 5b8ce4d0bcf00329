"""encode_mask_kernel's noise and the noise-aware decodes, bit for bit against the numpy restatement of the binomial
noise (tests/dp_cases.py): one batch of four clients with 0, 1, 5 and 14 seeds at every width, every b of the case
list, three lengths and both roundings, host and device forms with poisoned padding and guards; one batch of 0
through 17 seeds across the boundaries of the unit dealing; noise off is the existing calls byte for byte; the
refusals; whole rounds through flm_aggregate_unmask and the noise-aware decode, also through the store; the
reference-side binding."""
from __future__ import annotations

import functools
import hashlib
import importlib.util
import os

import numpy as np
import pytest

import codec_cases as K
import dp_cases as D
import pack_cases as PC

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POISON = 0xDEADBEEF


@pytest.fixture(scope="module")
def eng():
    from flamingo_amd import MaskEngine
    e = MaskEngine(0)
    yield e
    e.close()


def _u8(seeds32):
    return np.frombuffer(b"".join(seeds32), np.uint8).reshape(len(seeds32), 32).copy()


# ------------------------------------------------------------------ one batch, every case
@pytest.mark.parametrize("P,f,c,b", D.gpu_cases())
def test_batch_matches_the_restatement(eng, P, f, c, b):
    import torch
    N = len(D.BATCH_SEEDS)
    for L in D.LENGTHS:
        Lw = -(-L // P)
        xs, seg, seeds, signs, dithers, noises = D.batch(L, c, 7 * P + b)
        sd, nz, di = torch.from_numpy(seeds).cuda(), torch.from_numpy(_u8(noises)).cuda(), torch.from_numpy(_u8(dithers)).cuda()
        for d, dd in ((None, None), (dithers, di)):
            want, want_cl = D.batch_rows(xs, seg, seeds, signs, f, c, P, d, noises, b)
            _, plain_cl = eng.client_encode_noise_mask(seg, seeds, signs, L, xs, f, c, P, dither=d, return_clipped=True)
            assert plain_cl.sum() > 0 and np.array_equal(want_cl, plain_cl)       # the counts of the call without noise
            got, cl = eng.client_encode_noise_mask(seg, seeds, signs, L, xs, f, c, P, dither=d, noise_bits=b, noise=noises,
                                                   return_clipped=True)
            assert got.shape == (N, Lw) and np.array_equal(got, want), (L, "stochastic" if d else "nearest")
            assert np.array_equal(cl, want_cl), L
            # device form: x rows longer than L with NaN or 1e30 behind them, guard words behind each out row
            XP, OP = (L + 3) // 4 * 4 + 16, (Lw + 3) // 4 * 4 + 32
            for pad in (np.nan, 1e30):
                xp = np.full((N, XP), pad, np.float32)
                xp[:, :L] = xs
                xt = torch.from_numpy(xp).cuda()
                out = torch.full((N, OP), POISON - (1 << 32), dtype=torch.int32, device="cuda")
                clt = torch.full((N,), 77, dtype=torch.int32, device="cuda")
                eng.client_encode_noise_mask_dev(seg, sd, signs, out, L, xt, f, c, P, dither_dev=dd, noise_bits=b,
                                                 noise_dev=nz, clipped=clt)
                o = out.cpu().numpy().view(np.uint32)
                assert np.array_equal(o[:, :Lw], want), (L, pad)
                assert np.all(o[:, Lw:] == POISON)                              # guard words untouched
                assert np.array_equal(clt.cpu().numpy().view(np.uint32), want_cl)


# ------------------------------------------------------------------ the dealing boundaries
DEAL_CLIENTS = 18                                   # client i has i seeds, 0 through 17
DEAL_BITS = (0, 32, 64)                             # 0, P and 2 P noise units in front of the seeds


def _deal_params(P):
    return (16, 4.0) if P == 1 else PC.pack_params(P)       # P = 4: (2, 1.0), the one pair its fields admit


def _deal_cases():
    return [(P, st, b) for P in (1, 2, 4) for st in (False, True) for b in DEAL_BITS
            if D.headroom_ok(*_deal_params(P), P, b, 1)]


@functools.lru_cache(maxsize=None)
def _deal_batch(P):
    """The inputs of one width, built once: L = 1024 P + 1 parameters are two word tiles, the second of one word,
    whose upper fields (P > 1) lie past L."""
    f, c = _deal_params(P)
    L = 1024 * P + 1
    rng = np.random.default_rng(4100 + P)
    counts = np.arange(DEAL_CLIENTS)
    seeds = rng.integers(0, 256, size=(int(counts.sum()), 32), dtype=np.uint8)
    signs = rng.choice(np.array([-1, 1], np.int8), size=int(counts.sum()))
    seg = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    xs = np.stack([K.random_row(L, c, 4200 + 50 * P + i, wild=True) for i in range(DEAL_CLIENTS)])
    dithers = [hashlib.sha256(b"dp deal dither %d %d" % (P, i)).digest() for i in range(DEAL_CLIENTS)]
    noises = [D.seed(4300 + 100 * P + i) for i in range(DEAL_CLIENTS)]
    return f, c, L, xs, seg, seeds, signs, dithers, noises


@pytest.mark.parametrize("P,stochastic,b", _deal_cases())
def test_dealing_boundaries(eng, P, stochastic, b):
    """The unit list is dealt in threes up to unit 3 E (E = P stochastic, 1 nearest: 3, 6 or 12) and in fours from
    there, and with noise the P ceil(b / 32) noise units come first: with 0 through 17 seeds and b = 0, 32, 64 the
    change of step falls inside the noise units, on the first seed and among the seeds, and every wave's share ends
    before, on and after it.  Every word, the clipped counts and the guard words, against the restatement."""
    import torch
    f, c, L, xs, seg, seeds, signs, dithers, noises = _deal_batch(P)
    N, Lw = DEAL_CLIENTS, -(-L // P)
    assert Lw == 1025 and int(seg[-1]) == 153
    d = dithers if stochastic else None
    want, want_cl = D.batch_rows(xs, seg, seeds, signs, f, c, P, d, noises, b)
    XP, OP = (L + 3) // 4 * 4 + 16, (Lw + 3) // 4 * 4 + 32
    xp = np.full((N, XP), np.nan, np.float32)
    xp[:, :L] = xs
    out = torch.full((N, OP), POISON - (1 << 32), dtype=torch.int32, device="cuda")
    clt = torch.full((N,), 77, dtype=torch.int32, device="cuda")
    eng.client_encode_noise_mask_dev(seg, torch.from_numpy(seeds).cuda(), signs, out, L, torch.from_numpy(xp).cuda(), f, c, P,
                                     dither_dev=torch.from_numpy(_u8(dithers)).cuda() if stochastic else None, noise_bits=b,
                                     noise_dev=torch.from_numpy(_u8(noises)).cuda(), clipped=clt)
    o = out.cpu().numpy().view(np.uint32)
    bad = [i for i in range(N) if not np.array_equal(o[i, :Lw], want[i])]
    assert not bad, ("clients (= seed counts) whose rows differ", bad)
    assert np.all(o[:, Lw:] == POISON)                                      # guard words untouched
    assert want_cl.sum() > 0 and np.array_equal(clt.cpu().numpy().view(np.uint32), want_cl)


# ------------------------------------------------------------------ noise off
@pytest.mark.parametrize("P", (1, 2, 4))
def test_noise_off_is_the_existing_call(eng, P):
    import torch
    f, c = (16, 4.0) if P == 1 else PC.pack_params(P)
    L = 2077
    Lw = -(-L // P)
    xs, seg, seeds, signs, dithers, noises = D.batch(L, c, 90 + P)
    sd, nz, di = torch.from_numpy(seeds).cuda(), torch.from_numpy(_u8(noises)).cuda(), torch.from_numpy(_u8(dithers)).cuda()
    xt = torch.from_numpy(np.ascontiguousarray(np.pad(xs, ((0, 0), (0, 3))))).cuda()
    for d, dd in ((None, None), (dithers, di)):
        if P == 1:
            old, old_cl = eng.client_encode_mask(seg, seeds, signs, L, xs, f, c, dither=d, return_clipped=True)
        else:
            old, old_cl = eng.client_encode_pack_mask(seg, seeds, signs, L, xs, f, c, P, dither=d, return_clipped=True)
        assert np.array_equal(old, D.batch_rows(xs, seg, seeds, signs, f, c, P, d, None, 0)[0])
        for noise in (None, noises):                     # any noise pointer, NULL included
            new, new_cl = eng.client_encode_noise_mask(seg, seeds, signs, L, xs, f, c, P, dither=d, noise_bits=0, noise=noise,
                                                       return_clipped=True)
            assert new.tobytes() == old.tobytes() and new_cl.tobytes() == old_cl.tobytes()
        for noise_dev in (None, nz):
            out = torch.zeros((len(xs), Lw + 3 & ~3), dtype=torch.int32, device="cuda")
            eng.client_encode_noise_mask_dev(seg, sd, signs, out, L, xt, f, c, P, dither_dev=dd, noise_bits=0,
                                             noise_dev=noise_dev)
            assert np.array_equal(out.cpu().numpy().view(np.uint32)[:, :Lw], old)
    # and the decodes
    if P > 1:
        s = np.random.default_rng(P).integers(0, 2 ** 32, Lw, dtype=np.uint64).astype(np.uint32)
        assert eng.decode_unpack(s, L, f, c, P, 3, noise_bits=0).tobytes() == eng.decode_unpack(s, L, f, c, P, 3).tobytes()


# ------------------------------------------------------------------ refusals
def test_refusals_launch_nothing(eng):
    import torch
    from flamingo_amd._lib import p_f32, p_i64, p_i8, p_u8, p_u32
    seg = np.array([0, 1], np.int64)
    seeds, signs = _u8([D.seed(1)]), np.array([1], np.int8)
    noise = _u8([D.seed(2)])
    x = np.zeros((1, 8), np.float32)
    out = np.full(8, POISON, np.uint32)
    cl = np.full(1, 77, np.uint32)
    enc = eng.lib.flm_client_encode_noise_mask

    def call(f, c, P, b, nz):
        return enc(eng.ctx, p_f32(x), 1, p_i64(seg), p_u8(seeds), p_i8(signs), 8, f, c, P, None, b, nz, p_u32(out), p_u32(cl))

    assert call(4, 1.0, 2, 30, None) == -1 and b"noise" in eng.lib.flm_last_error(eng.ctx)      # noise_bits > 0, NULL noise
    assert call(4, 1.0, 1, 2, None) == -1
    for b in (1, 31, 1026, -2):
        assert call(4, 1.0, 2, b, p_u8(noise)) == -1, b
    assert call(4, 1.0, 3, 2, p_u8(noise)) == -1
    assert call(2, 1.0, 4, 248, p_u8(noise)) == -4 and call(7, 1.0, 4, 2, p_u8(noise)) == -4    # one client has no room
    assert np.all(out == POISON) and cl[0] == 77
    # the device form: refused before anything is launched or staged
    xt = torch.zeros((1, 8), dtype=torch.float32, device="cuda")
    ot = torch.full((1, 8), 5, dtype=torch.int32, device="cuda")
    sd = torch.from_numpy(seeds).cuda()
    with pytest.raises(RuntimeError, match="code -1"):
        eng.client_encode_noise_mask_dev(seg, sd, signs, ot, 8, xt, 4, 1.0, 2, noise_bits=30, noise_dev=None)
    torch.cuda.synchronize()
    assert np.all(ot.cpu().numpy() == 5)
    # the decodes: the noised headroom with n = count
    fo = np.full(8, 123.25, np.float32)
    dec = eng.lib.flm_decode_unpack_noise
    assert dec(eng.ctx, p_u32(out), 8, 4, 1.0, 2, 30, 1057, p_f32(fo)) == 0
    fo[:] = 123.25
    assert dec(eng.ctx, p_u32(out), 8, 4, 1.0, 2, 30, 1058, p_f32(fo)) == -4
    assert dec(eng.ctx, p_u32(out), 8, 4, 1.0, 2, 31, 1, p_f32(fo)) == -1
    assert dec(eng.ctx, p_u32(out), 8, 4, 1.0, 1, 30, 1, p_f32(fo)) == -1
    assert np.all(fo == np.float32(123.25))
    eng.codec_check(4, 1.0, 1057, pack=2, noise_bits=30, L=2077)
    with pytest.raises(RuntimeError, match="code -4"):
        eng.codec_check(4, 1.0, 1058, pack=2, noise_bits=30)


# ------------------------------------------------------------------ whole rounds
def _ring_graph(n_all, dropped, tag):
    """Self-mask and pair seeds on the graph i -- i +- 1, i +- 2 (mod n_all): every client's (seeds, signs), and the
    server's list that removes the survivors' self masks and their masks towards dropped neighbours."""
    pair = lambda a, b: hashlib.sha256(b"%s pair %d %d" % (tag, min(a, b), max(a, b))).digest()   # noqa: E731
    own = [hashlib.sha256(b"%s self %d" % (tag, i)).digest() for i in range(n_all)]
    nb = {i: sorted({(i + d) % n_all for d in (-2, -1, 1, 2)} - {i}) for i in range(n_all)}
    client = {i: ([own[i]] + [pair(i, j) for j in nb[i]], [1] + [1 if i < j else -1 for j in nb[i]]) for i in range(n_all)}
    useeds, usigns = [], []
    for i in range(n_all):
        if i in dropped:
            continue
        useeds.append(own[i]); usigns.append(-1)
        for j in nb[i]:
            if j in dropped:
                useeds.append(pair(i, j)); usigns.append(-1 if i < j else 1)
    return client, useeds, usigns


@pytest.mark.parametrize("f,c,P,b,n,L", D.GPU_ROUNDS)
def test_whole_round(eng, f, c, P, b, n, L):
    """n survivors (at P = 4 the most the noised headroom admits), every third at +c everywhere, mixed roundings; two
    more clients mask and drop, and their noise shares are simply absent.  The unmasked sum is the sum of the
    restatement's noised encodings, the decode is the restatement's bytes, and against the same round without noise
    the integer numerators differ by sum_i Z_i exactly: decoded = float32((numerator + sum_i Z_i) / (n 2^f))."""
    from flamingo_amd.ingest import VectorStore
    assert D.headroom_ok(f, c, P, b, n) and (P == 1 or not D.headroom_ok(f, c, P, b, n + 1))
    n_all, dropped = n + 2, {1, n}
    alive = [i for i in range(n_all) if i not in dropped]
    xs, dithers = PC.worst_inputs(f, c, n, L)
    x_of, d_of = dict(zip(alive, xs)), dict(zip(alive, dithers))
    for i in dropped:
        x_of[i], d_of[i] = K.random_row(L, c, 77 + i, wild=True), None
    z_of = {i: D.seed(500 + i) for i in range(n_all)}
    client, useeds, usigns = _ring_graph(n_all, dropped, b"dp %d" % P)

    def masked_rows(bits):
        rows = {}
        for stochastic in (False, True):             # a call rounds all its clients one way: two calls
            ids = [i for i in range(n_all) if (d_of[i] is not None) == stochastic]
            seg = np.concatenate([[0], np.cumsum([len(client[i][0]) for i in ids])]).astype(np.int64)
            seeds = [s for i in ids for s in client[i][0]]
            signs = [s for i in ids for s in client[i][1]]
            y = eng.client_encode_noise_mask(seg, seeds, signs, L, np.stack([x_of[i] for i in ids]), f, c, P,
                                             dither=[d_of[i] for i in ids] if stochastic else None, noise_bits=bits,
                                             noise=[z_of[i] for i in ids])
            rows.update(zip(ids, y))
        return np.stack([rows[i] for i in alive])

    rows = masked_rows(b)
    total = eng.aggregate_unmask(rows, useeds, usigns)
    enc = sum(D.encode_any(x_of[i], f, c, P, d_of[i], z_of[i], b)[0].astype(np.uint64) for i in alive)
    assert np.array_equal(total, (enc & 0xFFFFFFFF).astype(np.uint32))
    want = D.decode_any(total, L, f, c, P, b, n)
    mean = eng.decode_sum(total, f, n) if P == 1 else eng.decode_unpack(total, L, f, c, P, n, noise_bits=b)
    assert mean.dtype == np.float32 and mean.tobytes() == want.tobytes()

    plain = eng.aggregate_unmask(masked_rows(0), useeds, usigns)
    zsum = sum(D.noise(z_of[i], L, b) for i in alive)
    assert zsum.any() and np.abs(zsum).max() <= n * b // 2
    if P == 1:
        num0 = plain.view(np.int32).astype(np.int64)
        num = total.view(np.int32).astype(np.int64)
    else:
        W = 32 // P
        unpack = lambda S: ((S.astype(np.int64)[:, None] >> (W * np.arange(P, dtype=np.int64))) & (2 ** W - 1)).reshape(-1)[:L]  # noqa: E731
        num0 = unpack(plain) - n * PC.bias(f, c)
        num = unpack(total) - n * D.bias_n(f, c, b)
    assert np.array_equal(num - num0, zsum)
    assert mean.tobytes() == ((num0 + zsum).astype(np.float64) / (np.float64(n) * 2.0 ** f)).astype(np.float32).tobytes()

    if P > 1:                                           # the same through the store
        st = VectorStore(eng, -(-L // P), n)
        for k, i in enumerate(alive):
            st.add(i, rows[k])
        st.partial_sum()
        st.wait_partial()
        assert st.unmask_unpack_f32(useeds, usigns, L, f, c, P, n, noise_bits=b).tobytes() == want.tobytes()
        with pytest.raises(RuntimeError):                # one contributor more has no noised headroom
            st.unmask_unpack_f32(useeds, usigns, L, f, c, P, n + 1, noise_bits=b)
        st.close()


# ------------------------------------------------------------------ the reference-side binding
def test_reference_side_binding(eng, monkeypatch):
    """integration/util_flm.py's noise calls, once each, against the restatement."""
    monkeypatch.setenv("FLM_LIB", os.path.join(ROOT, "flamingo_amd", "lib", "libflamingo_hip.so"))
    import torch  # noqa: F401  (one HIP runtime per process: torch's, loaded first)
    spec = importlib.util.spec_from_file_location("util_flm", os.path.join(ROOT, "integration", "util_flm.py"))
    flm = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(flm)
    f, c, P, b, L = 4, 1.0, 2, 30, 1027
    xs, seg, seeds, signs, dithers, noises = D.batch(L, c, 3)
    flm.codec_check_noise(f, c, P, b, 1057, L)
    with pytest.raises(RuntimeError):
        flm.codec_check_noise(f, c, P, b, 1058)
    k0, k1 = int(seg[3]), int(seg[4])
    sd, sg = [bytes(s) for s in seeds[k0:k1]], list(signs[k0:k1])
    for pack in (1, P):
        want, want_cl = D.masked_noised(xs[3], f, c, pack, seeds[k0:k1], signs[k0:k1], dithers[3], noises[3], b)
        got, cl = flm.client_encode_noise_mask(sd, sg, L, xs[3], f, c, pack, dither=dithers[3], noise_bits=b, noise=noises[3])
        assert np.array_equal(got, want) and cl == want_cl
    s = np.random.default_rng(1).integers(0, 2 ** 32, -(-L // P), dtype=np.uint64).astype(np.uint32)
    assert flm.decode_unpack(s, L, f, c, P, 3, noise_bits=b).tobytes() == D.decode_packed_noised(s, L, f, c, P, b, 3).tobytes()
    st = flm.VectorStore(-(-L // P), 4)
    rows = np.random.default_rng(2).integers(0, 2 ** 32, (4, -(-L // P)), dtype=np.uint64).astype(np.uint32)
    for i in range(4):
        st.add(i, rows[i])
    st.partial()
    total = st.unmask(sd, sg)
    assert st.unmask_unpack_f32(sd, sg, L, f, c, P, 4, noise_bits=b).tobytes() == \
        D.decode_packed_noised(total, L, f, c, P, b, 4).tobytes()
