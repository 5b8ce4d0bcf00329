"""encode_mask_kernel at P = 2, 4 and decode_unpack_kernel, bit for bit against the numpy restatement of the packed codec
(tests/pack_cases.py), for 2 and 4 parameters per ring word, nearest and stochastic: every row-tail, word-tail and
tile shape, clients with 0..40 seeds mixed in one batch, the edge values in every field, the stochastic threshold
parameters (the dither stream is indexed by parameter), pitched device rows with poisoned padding and guards, the
decode's adjacent-field words and tails, the refusals, whole rounds at the largest cohort a width admits against
both the restatement and the unpacked path, the store's packed unmask on one engine and on three loopback ranks,
the reference-side binding, and one run of the agents."""
from __future__ import annotations

import hashlib
import importlib.util
import os

import numpy as np
import pytest

import codec_cases as K
import pack_cases as C

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COUNTS9 = (0, 0, 1, 3, 4, 5, 40, 0, 0)      # seeds per client, as tests/test_codec_gpu.py
POISON = 0xDEADBEEF


@pytest.fixture(scope="module")
def eng():
    from flamingo_amd import MaskEngine
    e = MaskEngine(0)
    yield e
    e.close()


def _seed(tag, i):
    return hashlib.sha256(f"pack {tag} {i}".encode()).digest()


def _batch(counts, tag):
    seg = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    n = int(seg[-1])
    seeds = np.frombuffer(b"".join(_seed(tag, k) for k in range(n)), np.uint8).reshape(n, 32).copy()
    signs = np.array([1 if (k * 7 + 3) % 5 < 3 else -1 for k in range(n)], np.int8)
    dither = [_seed(tag + " dither", i) for i in range(len(counts))]
    return seg, seeds, signs, dither


def _expect(x, seg, seeds, signs, f, c, P, dither):
    rows, cl = [], []
    for i in range(x.shape[0]):
        k0, k1 = int(seg[i]), int(seg[i + 1])
        r, n = C.masked_packed(x[i], f, c, P, seeds[k0:k1], signs[k0:k1], dither[i] if dither is not None else None)
        rows.append(r)
        cl.append(n)
    return np.stack(rows), np.array(cl, np.uint32)


# ------------------------------------------------------------------ encode
@pytest.mark.parametrize("N", [1, 9])
@pytest.mark.parametrize("P", C.PACKS)
def test_host_form_shapes(eng, P, N):
    f, c = C.pack_params(P)
    counts = COUNTS9 if N == 9 else (5,)
    for L in C.shapes(P):
        seg, seeds, signs, dither = _batch(counts, f"shape {P} {N} {L}")
        x = np.stack([K.random_row(L, c, 1000 * L + i, wild=True) for i in range(N)])
        for d in (None, dither):
            want, want_cl = _expect(x, seg, seeds, signs, f, c, P, d)
            got, cl = eng.client_encode_pack_mask(seg, seeds, signs, L, x, f, c, P, dither=d, return_clipped=True)
            assert got.shape == (N, -(-L // P)) and np.array_equal(got, want), (L, "stochastic" if d else "nearest")
            assert np.array_equal(cl, want_cl), L
            assert np.array_equal(eng.client_encode_pack_mask(seg, seeds, signs, L, x, f, c, P, dither=d), want)  # clipped NULL


@pytest.mark.parametrize("P", C.PACKS)
@pytest.mark.parametrize("f,c", C.VALUE_PARAMS)
def test_value_rows_in_every_field(eng, f, c, P):
    if not C.headroom_ok(f, c, P, 1):
        with pytest.raises(RuntimeError, match="code -4"):      # (7, 1) does not fit 8-bit fields at all
            eng.codec_check(f, c, 1, pack=P)
        return
    B, W = C.bias(f, c), 32 // P
    seg, seeds, signs, dither = _batch((3,), f"values {f} {P}")
    seg0, seeds0, signs0, _ = _batch((0,), "bare")
    for rot, v in enumerate(C.rotated_value_rows(f, c, P)):
        x, L = v[None, :], len(v)
        for d in (None, dither):
            want, want_cl = _expect(x, seg, seeds, signs, f, c, P, d)
            got, cl = eng.client_encode_pack_mask(seg, seeds, signs, L, x, f, c, P, dither=d, return_clipped=True)
            assert np.array_equal(got, want) and np.array_equal(cl, want_cl), rot
            # and bare, without masks: the words themselves
            bare = eng.client_encode_pack_mask(seg0, seeds0, signs0, L, x, f, c, P, dither=d[:1] if d else None)[0]
            assert np.array_equal(bare, C.encode_packed(v, f, c, P, d[0] if d else None)[0]), rot
            u = (bare[:, None].astype(np.int64) >> (W * np.arange(P))) & (2 ** W - 1)
            u = u.reshape(-1)
            assert u[:L].max() <= 2 * B and np.all(u[L:] == 0)           # no bit outside a field's range
            top, bottom = (8 + rot) % L, (9 + rot) % L                    # value_row's +c and -c
            assert u[top] == 2 * B and u[bottom] == 0


@pytest.mark.parametrize("P", C.PACKS)
def test_stochastic_threshold_parameters(eng, P):
    """The threshold row is made for (f = 7, c = 1), where P = 4 has no headroom: P = 4 runs at f = 2 with the picked
    parameters scaled by 2^5 (exact), so that their t = x 2^f, and with it the threshold, is the same."""
    x, picks = C.threshold_row()
    f = C.THRESHOLD_F if P == 2 else 2
    if P == 4:
        x = x.copy()
        for l, *_ in picks:
            x[l] = x[l] * np.float32(2.0 ** (C.THRESHOLD_F - 2))
    seg, seeds, signs, _ = _batch((0,), "thr")
    got = eng.client_encode_pack_mask(seg, seeds, signs, len(x), x[None, :], f, C.THRESHOLD_C, P, dither=[C.DITHER])[0]
    assert np.array_equal(got, C.encode_packed(x, f, C.THRESHOLD_C, P, C.DITHER)[0])
    W, B = 32 // P, C.bias(f, C.THRESHOLD_C)
    for l, _, _, away in picks:
        q = int((int(got[l // P]) >> (W * (l % P))) & (2 ** W - 1)) - B
        assert q == (int(np.sign(x[l])) if away else 0), (l, away)


@pytest.mark.parametrize("P", C.PACKS)
def test_dev_form_pitches_padding_guards_and_streams(eng, P):
    import torch
    f, c = C.pack_params(P)
    N, L = 9, 2077 * P + P - 1
    Lw = -(-L // P)
    XP, OP = (L + 3) // 4 * 4 + 16, (Lw + 3) // 4 * 4 + 32
    seg, seeds, signs, dither = _batch(COUNTS9, f"dev {P}")
    x = np.clip(np.stack([K.random_row(L, 0.8 * c, 50 + i) for i in range(N)]), -c, c)
    # clipped elements in the first, a middle and the last tile of a row: the count sums over workgroups
    x[2, [0, 5]] = 9.0
    x[2, 1024 * P + 7] = np.nan
    x[2, L - 1] = -np.inf
    x[6, 2048 * P] = np.nextafter(np.float32(c), np.float32(np.inf))
    x[8, 1023] = -5.0
    sd = torch.from_numpy(seeds).cuda()
    di = torch.from_numpy(np.frombuffer(b"".join(dither), np.uint8).reshape(N, 32).copy()).cuda()
    side = torch.cuda.Stream()
    for d, dd in ((None, None), (dither, di)):
        want, want_cl = _expect(x, seg, seeds, signs, f, c, P, d)
        assert list(want_cl) == [0, 0, 4, 0, 0, 0, 1, 0, 1]
        results = []
        for pad, stream in ((np.nan, None), (1e30, None), (1e30, side)):
            xp = np.full((N, XP), pad, np.float32)
            xp[:, :L] = x
            xt = torch.from_numpy(xp).cuda()
            out = torch.full((N, OP), POISON - (1 << 32), dtype=torch.int32, device="cuda")
            cl = torch.full((N,), 77, dtype=torch.int32, device="cuda")
            if stream is not None:
                stream.wait_stream(torch.cuda.current_stream())
            eng.client_encode_pack_mask_dev(seg, sd, signs, out, L, xt, f, c, P, dither_dev=dd, clipped=cl, stream=stream)
            if stream is not None:
                stream.synchronize()
            o = out.cpu().numpy().view(np.uint32)
            assert np.array_equal(o[:, :Lw], want)
            assert np.all(o[:, Lw:] == POISON)                      # guard words untouched
            assert np.array_equal(cl.cpu().numpy().view(np.uint32), want_cl)
            results.append(o.tobytes())
        assert results[0] == results[1] == results[2]
        # clipped = NULL
        xt = torch.from_numpy(np.ascontiguousarray(np.pad(x, ((0, 0), (0, XP - L))))).cuda()
        out = torch.zeros((N, OP), dtype=torch.int32, device="cuda")
        eng.client_encode_pack_mask_dev(seg, sd, signs, out, L, xt, f, c, P, dither_dev=dd)
        assert np.array_equal(out.cpu().numpy().view(np.uint32)[:, :Lw], want)


# ------------------------------------------------------------------ decode
@pytest.mark.parametrize("P", C.PACKS)
def test_decode_unpack(eng, P):
    import torch
    f, c = C.pack_params(P)
    for L in list(range(1, 4 * P + 2)) + [16 * P + 3, 1024 * P + P + 1, 2077 * P - 1]:    # every remainder mod P and 4
        Lw = -(-L // P)
        rng = np.random.default_rng(L)
        s = rng.integers(0, 2 ** 32, Lw, dtype=np.uint64).astype(np.uint32)
        s[:min(Lw, 6)] = C.DECODE_WORDS[:min(Lw, 6)]
        for n in C.decode_counts(P):
            want = C.decode_packed(s, L, f, c, P, n)
            assert eng.decode_unpack(s, L, f, c, P, n).tobytes() == want.tobytes(), (L, n)
            t = torch.from_numpy(s.view(np.int32).copy()).cuda()
            o = torch.full((L + 9,), 123.25, dtype=torch.float32, device="cuda")
            eng.decode_unpack_dev(t, o, L, f, c, P, n)
            o = o.cpu().numpy()
            assert o[:L].tobytes() == want.tobytes(), (L, n)
            assert np.all(o[L:] == np.float32(123.25))                   # guard floats behind L untouched
            assert np.array_equal(t.cpu().numpy().view(np.uint32), s)    # and the sum is still the sum


@pytest.mark.parametrize("P", C.PACKS)
def test_decode_adjacent_field_words_exact(eng, P):
    f, c = C.pack_params(P)
    L = len(C.DECODE_WORDS) * P
    for n in C.decode_counts(P):
        got = eng.decode_unpack(C.DECODE_WORDS, L, f, c, P, n)
        assert got.tobytes() == C.decode_packed(C.DECODE_WORDS, L, f, c, P, n).tobytes()
    # a field at 2^W - 1 beside one at 0, one contributor: exactly (2^W - 1 - B) / 2^f and -B / 2^f
    B, top = C.bias(f, c), 2 ** (32 // P) - 1
    got = eng.decode_unpack(C.DECODE_WORDS[:1], P, f, c, P, 1)            # 0xFFFF0000
    want = [-B / 2.0 ** f] * (P // 2) + [(top - B) / 2.0 ** f] * (P // 2)
    assert list(got) == [np.float32(v) for v in want]


# ------------------------------------------------------------------ refusals
def test_refusals(eng):
    from flamingo_amd._lib import p_f32, p_i64, p_i8, p_u8, p_u32
    seg, seeds, signs, _ = _batch((1,), "refuse")
    x = np.zeros((1, 8), np.float32)
    out = np.full(8, POISON, np.uint32)
    cl = np.full(1, 77, np.uint32)
    fo = np.full(8, 123.25, np.float32)
    enc, dec = eng.lib.flm_client_encode_pack_mask, eng.lib.flm_decode_unpack

    def untouched():
        return np.all(out == POISON) and cl[0] == 77 and np.all(fo == np.float32(123.25))

    for pack in (0, 1, 3, 8):
        assert enc(eng.ctx, p_f32(x), 1, p_i64(seg), p_u8(seeds), p_i8(signs), 8, 7, 1.0, pack, None, p_u32(out),
                   p_u32(cl)) == -1
        assert dec(eng.ctx, p_u32(out), 8, 7, 1.0, pack, 1, p_f32(fo)) == -1
        assert eng.lib.flm_codec_check_packed(7, 1.0, pack, 1) == -1
        assert untouched()
    for f, c, P, n in C.HEADROOM_EDGES:
        eng.codec_check(f, c, n, pack=P)
        with pytest.raises(RuntimeError, match="code -4"):
            eng.codec_check(f, c, n + 1, pack=P)
        w = np.zeros(2, np.uint32)
        eng.decode_unpack(w, 2 * P, f, c, P, n)                                   # at the edge: passes
        assert dec(eng.ctx, p_u32(out), 8, f, c, P, n + 1, p_f32(fo)) == -4       # one step past it
        assert untouched()
    # the encode applies the rule with n = 1: (7, 1) has no 8-bit field, (15, 1) no 16-bit one
    for f, P in ((7, 4), (15, 2)):
        assert enc(eng.ctx, p_f32(x), 1, p_i64(seg), p_u8(seeds), p_i8(signs), 8, f, 1.0, P, None, p_u32(out),
                   p_u32(cl)) == -4
    assert enc(eng.ctx, p_f32(x), 1, p_i64(seg), p_u8(seeds), p_i8(signs), 8, 31, 1.0, 2, None, p_u32(out), p_u32(cl)) == -1
    assert enc(eng.ctx, None, 1, p_i64(seg), p_u8(seeds), p_i8(signs), 8, 7, 1.0, 2, None, p_u32(out), p_u32(cl)) == -1
    assert dec(eng.ctx, None, 8, 7, 1.0, 2, 1, p_f32(fo)) == -1
    assert dec(eng.ctx, p_u32(out), 8, 7, 1.0, 2, 0, p_f32(fo)) == -1
    assert untouched()
    # pack = 1 through the engine is the unpacked call
    eng.codec_check(16, 4.0, 8191, pack=1)
    with pytest.raises(RuntimeError, match="code -4"):
        eng.codec_check(16, 4.0, 8192, pack=1)


def test_dev_form_refuses_short_pitches(eng):
    import torch
    seg, seeds, signs, _ = _batch((1,), "pitch")
    sd = torch.from_numpy(seeds).cuda()
    L, P = 21, 2                                       # 11 words: the out pitch must be at least 12
    x = torch.zeros((2, 24), dtype=torch.float32, device="cuda")
    out = torch.full((2, 12), 5, dtype=torch.int32, device="cuda")
    seg2 = np.array([0, 1, 1], np.int64)
    eng.client_encode_pack_mask_dev(seg2, sd, signs, out, L, x, 7, 1.0, P)
    import ctypes
    from flamingo_amd._lib import p_i64, p_i8
    dev = eng.lib.flm_client_encode_pack_mask_dev
    args = lambda xp, op: (eng.ctx, ctypes.c_void_p(x.data_ptr()), xp, 2, p_i64(seg2), ctypes.c_void_p(sd.data_ptr()),  # noqa: E731
                           p_i8(signs), L, 7, 1.0, P, None, ctypes.c_void_p(out.data_ptr()), op, None, None)
    before = out.cpu().numpy().copy()
    assert dev(*args(20, 12)) == -1 and dev(*args(24, 8)) == -1 and dev(*args(24, 11)) == -1 and dev(*args(22, 12)) == -1
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), before)


# ------------------------------------------------------------------ whole rounds at the worst case
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


@pytest.mark.parametrize("f,c,P,n,L", C.GPU_ROUNDS)
def test_whole_round_at_the_largest_cohort(eng, f, c, P, n, L):
    """n survivors, the most the width admits, every third at +c everywhere, mixed roundings; three more clients
    mask and drop.  client_encode_pack_mask -> aggregate_unmask -> decode_unpack is the restatement's bytes, and the
    bytes of client_encode_mask -> the same round over L words -> decode_sum."""
    assert C.headroom_ok(f, c, P, n) and not C.headroom_ok(f, c, P, n + 1)
    n_all, dropped = n + 3, {1, 57 % n, n + 1}
    alive = [i for i in range(n_all) if i not in dropped]
    xs, dithers = C.worst_inputs(f, c, n, L)
    x_of, d_of = dict(zip(alive, xs)), dict(zip(alive, dithers))
    for i in dropped:
        x_of[i], d_of[i] = K.random_row(L, c, 77 + i, wild=True), None
    client, useeds, usigns = _ring_graph(n_all, dropped, b"worst %d" % P)

    def masked_rows(packed):
        rows = {}
        for stochastic in (False, True):             # a call rounds all its clients one way: two calls
            ids = [i for i in range(n_all) if (d_of[i] is not None) == stochastic]
            seg = np.concatenate([[0], np.cumsum([len(client[i][0]) for i in ids])]).astype(np.int64)
            seeds = [s for i in ids for s in client[i][0]]
            signs = [s for i in ids for s in client[i][1]]
            x = np.stack([x_of[i] for i in ids])
            d = [d_of[i] for i in ids] if stochastic else None
            y = eng.client_encode_pack_mask(seg, seeds, signs, L, x, f, c, P, dither=d) if packed \
                else eng.client_encode_mask(seg, seeds, signs, L, x, f, c, dither=d)
            rows.update(zip(ids, y))
        return np.stack([rows[i] for i in alive])

    total = eng.aggregate_unmask(masked_rows(True), useeds, usigns)
    enc = sum(C.encode_packed(x_of[i], f, c, P, d_of[i])[0].astype(np.uint64) for i in alive)
    assert int(enc.max()) < 2 ** 32 and np.array_equal(total, enc.astype(np.uint32))
    mean = eng.decode_unpack(total, L, f, c, P, n)
    assert mean.tobytes() == C.decode_packed(enc.astype(np.uint32), L, f, c, P, n).tobytes()
    plain = eng.aggregate_unmask(masked_rows(False), useeds, usigns)
    assert plain.shape == (L,) and mean.tobytes() == eng.decode_sum(plain, f, n).tobytes()


# ------------------------------------------------------------------ the store
@pytest.mark.parametrize("G", [1, 3])
@pytest.mark.parametrize("P", C.PACKS)
def test_store_unmask_unpack_f32(P, G):
    from flamingo_amd import DeviceGroup, MaskEngine
    from flamingo_amd._lib import p_f32, p_i8, p_u8
    from flamingo_amd.ingest import VectorStore
    f, c = C.pack_params(P)
    N, Lp, n_seeds = 8, 2077 * P - 1, 11            # shard edges fall inside words' parameter runs
    Lw = -(-Lp // P)
    rng = np.random.default_rng(10 * P + G)
    rows = rng.integers(0, 2 ** 32, (N, Lw), dtype=np.uint64).astype(np.uint32)
    _, seeds, signs, _ = _batch((n_seeds,), f"store {P} {G}")
    e = MaskEngine(0) if G == 1 else DeviceGroup([0] * G)
    try:
        st = VectorStore(e, Lw, N)
        for i in range(N):
            st.add(i, rows[i])
        st.partial_sum()
        st.wait_partial()
        total = st.unmask(seeds, signs)
        for n in (N, 1, C.decode_counts(P)[-1]):
            got = st.unmask_unpack_f32(seeds, signs, Lp, f, c, P, n)
            assert got.shape == (Lp,) and got.tobytes() == C.decode_packed(total, Lp, f, c, P, n).tobytes(), n
        assert np.array_equal(st.unmask(seeds, signs), total)           # the sum itself is still there
        out = np.full(Lp + 2, 123.25, np.float32)

        def code(L_params, pack, count):
            return st.lib.flm_store_unmask_unpack_f32(st.h, p_u8(seeds), p_i8(signs), n_seeds, L_params, f, c, pack, count,
                                                      p_f32(out))

        for bad_len in (Lp + 2, Lp - P, Lw):                            # not this store's ceil(L_params / pack)
            assert code(bad_len, P, N) == -1, bad_len
        assert code(Lp, 3, N) == -1 and code(Lp, P, 0) == -1
        assert code(Lp, P, C.decode_counts(P)[-1] + 1) == -4
        assert np.all(out == np.float32(123.25))                        # nothing is written on a refusal
        with pytest.raises(RuntimeError, match="ceil"):
            st.unmask_unpack_f32(seeds, signs, Lp + 2, f, c, P, N)
        st.close()
    finally:
        e.close()


# ------------------------------------------------------------------ the reference-side binding
def test_reference_side_binding(eng, monkeypatch):
    """integration/util_flm.py's four packed calls, once each, against the engine's."""
    monkeypatch.setenv("FLM_LIB", os.path.join(ROOT, "flamingo_amd", "lib", "libflamingo_hip.so"))
    import torch  # noqa: F401  (one HIP runtime per process: torch's, loaded first)
    spec = importlib.util.spec_from_file_location("util_flm", os.path.join(ROOT, "integration", "util_flm.py"))
    flm = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(flm)
    P, L = 2, 1027
    f, c = C.pack_params(P)
    seg, seeds, signs, dither = _batch((4,), "binding")
    x = K.random_row(L, c, 3, wild=True)
    flm.codec_check_packed(f, c, P, 255)
    with pytest.raises(RuntimeError):
        flm.codec_check_packed(f, c, P, 256)
    want, want_cl = eng.client_encode_pack_mask(seg, seeds, signs, L, x[None, :], f, c, P, dither=dither[:1],
                                                return_clipped=True)
    got, cl = flm.client_encode_pack_mask([bytes(s) for s in seeds], list(signs), L, x, f, c, P, dither=dither[0])
    assert np.array_equal(got, want[0]) and cl == int(want_cl[0])
    s = np.random.default_rng(1).integers(0, 2 ** 32, -(-L // P), dtype=np.uint64).astype(np.uint32)
    assert flm.decode_unpack(s, L, f, c, P, 3).tobytes() == eng.decode_unpack(s, L, f, c, P, 3).tobytes()
    st = flm.VectorStore(-(-L // P), 4)
    rows = np.random.default_rng(2).integers(0, 2 ** 32, (4, -(-L // P)), dtype=np.uint64).astype(np.uint32)
    for i in range(4):
        st.add(i, rows[i])
    st.partial()
    us, ug = [bytes(s) for s in seeds], list(signs)
    total = st.unmask(us, ug)
    assert st.unmask_unpack_f32(us, ug, L, f, c, P, 4).tobytes() == C.decode_packed(total, L, f, c, P, 4).tobytes()


# ------------------------------------------------------------------ the agents
def test_packed_float_inputs_through_the_agents():
    """n = 32, 4097 parameters in 2049 words, stochastic rounding, two iterations with three clients offline:
    final_mean (VectorStore.unmask_unpack_f32) is the restatement's decode of the sum of the online clients' packed
    encodings; the encodings themselves are checked in the last iteration, whose dither seeds the clients keep."""
    from flamingo_amd.abides.config_flamingo import run
    from flamingo_amd.abides.flamingo import protocol
    f, c, P, L = 7, 1.0, 2, 4097
    try:
        res = run(["-c", "flamingo", "-n", "32", "-i", "2", "-s", "11", "-k", "--offline", "3,17,30",
                   "--committee_size", "9", "--vector_len", str(L), "--float_inputs", "7,1,sr,pack2"])
        assert protocol.codec_pack() == 2 and protocol.ring_len() == 2049
    finally:
        protocol.configure(codec=False)
    srv, clients = res["server"], res["clients"]
    assert sorted(srv.means) == [1, 2]
    assert len(srv.recon_symbol) > 0          # dropout pairs were cancelled
    for it in (1, 2):
        ids = srv.online_ids[it]
        assert 0 < len(ids) == srv.online_counts[it] <= 29
        mean, total = srv.means[it], srv.results[it]
        assert mean.dtype == np.float32 and mean.shape == (L,) and total.dtype == np.uint32 and total.shape == (2049,)
        assert mean.tobytes() == C.decode_packed(total, L, f, c, P, len(ids)).tobytes()
        xs = [np.asarray(clients[i].input_vector, np.float32) for i in ids]
        assert all(clients[i].clipped == 0 for i in ids)
        if it == 2:
            assert all(clients[i].dither_seed is not None for i in ids)
            enc = sum(C.encode_packed(x, f, c, P, clients[i].dither_seed)[0].astype(np.uint64)
                      for i, x in zip(ids, xs)).astype(np.uint32)
            assert np.array_equal(total, enc)
            assert mean.tobytes() == C.decode_packed(enc, L, f, c, P, len(ids)).tobytes()
        exact = np.mean([x.astype(np.float64) for x in xs], axis=0)
        err = np.abs(mean.astype(np.float64) - exact)
        assert np.all(err <= 2.0 ** -f + 2.0 ** -24 * np.abs(exact)), float(err.max())
