"""encode_mask_kernel and decode_sum_kernel, bit for bit against the numpy restatement of the codec
(tests/codec_cases.py): every row-tail and tile shape, clients with 0..40 seeds mixed in one batch, the edge
values under both roundings, the stochastic threshold slots, pitched device rows with poisoned padding, the
clip counts summed over workgroups, both host routes, the store's float unmask and one whole round trip."""
from __future__ import annotations

import hashlib

import numpy as np
import pytest

import codec_cases as C

pytestmark = pytest.mark.gpu

LS = (1, 15, 16, 17, 1023, 1024, 1025, 2077)
COUNTS9 = (0, 0, 1, 3, 4, 5, 40, 0, 0)      # seeds per client: empty clients first, last and adjacent
POISON = 0xDEADBEEF


@pytest.fixture(scope="module")
def eng():
    from flamingo_amd import MaskEngine
    e = MaskEngine(0)
    yield e
    e.close()


def _seed(tag, i):
    return hashlib.sha256(f"codec {tag} {i}".encode()).digest()


def _batch(counts, tag):
    seg = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    K = int(seg[-1])
    seeds = np.frombuffer(b"".join(_seed(tag, k) for k in range(K)), np.uint8).reshape(K, 32).copy()
    signs = np.array([1 if (k * 7 + 3) % 5 < 3 else -1 for k in range(K)], np.int8)
    dither = [_seed(tag + " dither", i) for i in range(len(counts))]
    return seg, seeds, signs, dither


def _expect(x, seg, seeds, signs, f, c, dither):
    rows, cl = [], []
    for i in range(x.shape[0]):
        k0, k1 = int(seg[i]), int(seg[i + 1])
        r, n = C.masked(x[i], f, c, seeds[k0:k1], signs[k0:k1], dither[i] if dither is not None else None)
        rows.append(r)
        cl.append(n)
    return np.stack(rows), np.array(cl, np.uint32)


@pytest.mark.parametrize("N", [1, 9])
@pytest.mark.parametrize("L", LS)
def test_host_form_shapes(eng, N, L):
    counts = COUNTS9 if N == 9 else (5,)
    seg, seeds, signs, dither = _batch(counts, f"shape {N} {L}")
    x = np.stack([C.random_row(L, 4.0, 1000 * L + i, wild=True) for i in range(N)])
    for d in (None, dither):
        want, want_cl = _expect(x, seg, seeds, signs, 16, 4.0, d)
        got, cl = eng.client_encode_mask(seg, seeds, signs, L, x, 16, 4.0, dither=d, return_clipped=True)
        assert np.array_equal(got, want), ("stochastic" if d else "nearest")
        assert np.array_equal(cl, want_cl)
        assert np.array_equal(eng.client_encode_mask(seg, seeds, signs, L, x, 16, 4.0, dither=d), want)  # clipped NULL


def test_no_seeds_at_all(eng):
    seg, seeds, signs, dither = _batch((0, 0, 0), "k0")
    x = np.stack([C.random_row(1025, 4.0, i) for i in range(3)])
    for d in (None, dither):
        want, _ = _expect(x, seg, seeds, signs, 16, 4.0, d)
        assert np.array_equal(eng.client_encode_mask(seg, seeds, signs, 1025, x, 16, 4.0, dither=d), want)


@pytest.mark.parametrize("f,c", C.PARAMS)
def test_value_rows(eng, f, c):
    x = C.value_row(f, c)[None, :]
    seg, seeds, signs, dither = _batch((3,), f"values {f}")
    for d in (None, dither):
        want, want_cl = _expect(x, seg, seeds, signs, f, c, d)
        got, cl = eng.client_encode_mask(seg, seeds, signs, x.shape[1], x, f, c, dither=d, return_clipped=True)
        assert np.array_equal(got, want) and np.array_equal(cl, want_cl)
    # and bare, without masks: the words themselves
    seg0, seeds0, signs0, _ = _batch((0,), "bare")
    got = eng.client_encode_mask(seg0, seeds0, signs0, x.shape[1], x, f, c)
    assert np.array_equal(got[0], C.encode(x[0], f, c)[0])


def test_stochastic_threshold_slots(eng):
    x, picks = C.threshold_row()
    seg, seeds, signs, _ = _batch((0,), "thr")
    got = eng.client_encode_mask(seg, seeds, signs, C.THRESHOLD_L, x[None, :], C.THRESHOLD_F, C.THRESHOLD_C,
                                 dither=[C.DITHER])[0]
    assert np.array_equal(got, C.encode(x, C.THRESHOLD_F, C.THRESHOLD_C, C.DITHER)[0])
    q = got.view(np.int32)
    for l, _, _, away in picks:
        assert q[l] == (int(np.sign(x[l])) if away else 0)


def test_refusals(eng):
    seg, seeds, signs, _ = _batch((1,), "refuse")
    x = np.zeros((1, 8), np.float32)
    for f, c in ((-1, 1.0), (31, 1.0), (16, 0.0), (16, float("inf")), (16, float("nan"))):
        with pytest.raises(RuntimeError, match="code -1"):
            eng.client_encode_mask(seg, seeds, signs, 8, x, f, c)
    with pytest.raises(RuntimeError, match="code -4"):
        eng.client_encode_mask(seg, seeds, signs, 8, x, 30, 2.5)
    with pytest.raises(RuntimeError, match="code -4"):
        eng.codec_check(16, 4.0, 8192)
    eng.codec_check(16, 4.0, 8191)
    with pytest.raises(RuntimeError, match="code -1"):
        eng.decode_sum(np.zeros(4, np.uint32), 16, 0)
    from flamingo_amd._lib import p_i64, p_i8, p_u8, p_u32
    out = np.zeros(8, np.uint32)
    assert eng.lib.flm_client_encode_mask(eng.ctx, None, 1, p_i64(seg), p_u8(seeds), p_i8(signs), 8, 16, 4.0, None,
                                          p_u32(out), None) == -1


def test_dev_form_pitches_padding_guards_and_streams(eng):
    import torch
    N, L, XP, OP, f, c = 9, 2077, 2096, 2112, 16, 4.0
    seg, seeds, signs, dither = _batch(COUNTS9, "dev")
    x = np.stack([C.random_row(L, 3.0, 50 + i) for i in range(N)])
    x = np.clip(x, -c, c)
    # clipped elements in the first, a middle and the last tile of a row: the count sums over workgroups
    x[2, [0, 5]] = 9.0
    x[2, 1024 + 7] = np.nan
    x[2, 2076] = -np.inf
    x[6, 2048] = 4.0000005
    x[8, 1023] = -5.0
    sd = torch.from_numpy(seeds).cuda()
    di = torch.from_numpy(np.frombuffer(b"".join(dither), np.uint8).reshape(N, 32).copy()).cuda()
    side = torch.cuda.Stream()
    for d, dd in ((None, None), (dither, di)):
        want, want_cl = _expect(x, seg, seeds, signs, f, c, d)
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
            eng.client_encode_mask_dev(seg, sd, signs, out, L, xt, f, c, dither_dev=dd, clipped=cl, stream=stream)
            if stream is not None:
                stream.synchronize()
            o = out.cpu().numpy().view(np.uint32)
            assert np.array_equal(o[:, :L], want)
            assert np.all(o[:, L:] == POISON)                       # guard words untouched
            assert np.array_equal(cl.cpu().numpy().view(np.uint32), want_cl)
            results.append(o.tobytes())
        assert results[0] == results[1] == results[2]
        # clipped = NULL
        xt = torch.from_numpy(np.ascontiguousarray(np.pad(x, ((0, 0), (0, XP - L))))).cuda()
        out = torch.zeros((N, OP), dtype=torch.int32, device="cuda")
        eng.client_encode_mask_dev(seg, sd, signs, out, L, xt, f, c, dither_dev=dd)
        assert np.array_equal(out.cpu().numpy().view(np.uint32)[:, :L], want)


def test_agrees_with_client_mask_of_the_encoded_words(eng):
    N, L = 9, 1025
    seg, seeds, signs, dither = _batch(COUNTS9, "agree")
    x = np.stack([C.random_row(L, 4.0, 7 + i, wild=True) for i in range(N)])
    for d in (None, dither):
        enc = np.stack([C.encode(x[i], 16, 4.0, d[i] if d else None)[0] for i in range(N)])
        assert np.array_equal(eng.client_encode_mask(seg, seeds, signs, L, x, 16, 4.0, dither=d),
                              eng.client_mask(seg, seeds, signs, L, x=enc))


@pytest.mark.parametrize("L", [(1 << 16) + 3, (1 << 23) + 5])
def test_host_form_one_client_both_routes(eng, L):
    """N = 1 (the agents' call) below and above the size to which the host form runs in place in the pinned buffer."""
    seg, seeds, signs, dither = _batch((2,), f"route {L}")
    x = C.random_row(L, 4.0, L, wild=True)[None, :]
    want, want_cl = _expect(x, seg, seeds, signs, 16, 4.0, None)
    got, cl = eng.client_encode_mask(seg, seeds, signs, L, x, 16, 4.0, return_clipped=True)
    assert np.array_equal(got, want) and np.array_equal(cl, want_cl)


@pytest.mark.parametrize("L", [1, 3, 4, 5, 1025])
def test_decode_sum(eng, L):
    import torch
    rng = np.random.default_rng(L)
    s = rng.integers(0, 2 ** 32, L, dtype=np.uint64).astype(np.uint32)
    s[:min(L, 6)] = C.DECODE_WORDS[:min(L, 6)]
    for f in (0, 16, 30):
        for n in C.DECODE_COUNTS:
            want = C.decode(s, f, n)
            assert eng.decode_sum(s, f, n).tobytes() == want.tobytes()
            t = torch.from_numpy(s.view(np.int32).copy()).cuda()
            o = torch.zeros(L, dtype=torch.float32, device="cuda")
            eng.decode_sum_dev(t, o, L, f, n)
            assert o.cpu().numpy().tobytes() == want.tobytes()
            eng.decode_sum_dev(t, t.view(torch.float32), L, f, n)          # in place
            assert t.cpu().numpy().tobytes() == want.tobytes()


def test_decode_cases_exact(eng):
    for f in (0, 16, 30):
        for n in C.DECODE_COUNTS:
            assert eng.decode_sum(C.DECODE_WORDS, f, n).tobytes() == C.decode(C.DECODE_WORDS, f, n).tobytes()


@pytest.mark.parametrize("G", [1, 3])
def test_store_unmask_f32(G):
    from flamingo_amd import DeviceGroup, MaskEngine
    from flamingo_amd.ingest import VectorStore
    N, L, K = 8, 1000, 11
    rng = np.random.default_rng(G)
    rows = rng.integers(0, 2 ** 32, (N, L), dtype=np.uint64).astype(np.uint32)
    _, seeds, signs, _ = _batch((K,), f"store {G}")
    e = MaskEngine(0) if G == 1 else DeviceGroup([0] * G)
    try:
        st = VectorStore(e, L, N)
        for i in range(N):
            st.add(i, rows[i])
        st.partial_sum()
        st.wait_partial()
        total = st.unmask(seeds, signs)
        for f, n in ((16, N), (0, 1), (30, 3)):
            assert st.unmask_f32(seeds, signs, f, n).tobytes() == C.decode(total, f, n).tobytes()
        assert np.array_equal(st.unmask(seeds, signs), total)           # the sum itself is still there
        with pytest.raises(RuntimeError):
            st.unmask_f32(seeds, signs, 16, 0)
        st.close()
    finally:
        e.close()


def test_round_trip_with_dropouts(eng):
    """N = 8 clients on the protocol's neighbour graph, two of them drop after masking: the survivors' rows,
    the dropped clients' pair masks and the survivors' self masks give the mean of the survivors' floats."""
    import oracle
    N, L, f, c = 8, 1000, 16, 4.0
    root = hashlib.sha256(b"codec round trip").digest()
    x = np.clip(np.stack([C.random_row(L, c, 900 + i) for i in range(N)]), -c, c)     # nothing clips
    nb = {i: sorted(oracle.find_neighbors(root, 1, N, i, 4)) for i in range(N)}
    for i in range(N):                                               # the graph is symmetric: masks cancel in pairs
        assert all(i in nb[j] for j in nb[i])
    pair = lambda a, b: hashlib.sha256(b"pair %d %d" % (min(a, b), max(a, b))).digest()   # noqa: E731
    own = [hashlib.sha256(b"self %d" % i).digest() for i in range(N)]
    counts, seeds, signs = [], [], []
    for i in range(N):
        counts.append(1 + len(nb[i]))
        seeds.append(own[i]); signs.append(1)
        for j in nb[i]:
            seeds.append(pair(i, j)); signs.append(1 if i < j else -1)
    seg = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    y = eng.client_encode_mask(seg, seeds, signs, L, x, f, c)
    dropped = {2, 5}
    alive = [i for i in range(N) if i not in dropped]
    useeds, usigns = [], []
    for i in alive:
        useeds.append(own[i]); usigns.append(-1)
        for j in nb[i]:
            if j in dropped:                                         # i's mask towards a dropped neighbour stays: remove it
                useeds.append(pair(i, j)); usigns.append(-1 if i < j else 1)
    total = eng.aggregate_unmask(y[alive], useeds, usigns)
    enc = sum(C.encode(x[i], f, c)[0].astype(np.uint64) for i in alive).astype(np.uint32)
    assert np.array_equal(total, enc)
    mean = eng.decode_sum(total, f, len(alive))
    assert mean.tobytes() == C.decode(enc, f, len(alive)).tobytes()
    exact = x[alive].astype(np.float64).mean(axis=0)
    assert np.all(np.abs(mean.astype(np.float64) - exact) <= 2.0 ** -(f + 1) + 2.0 ** -24 * np.abs(exact))
