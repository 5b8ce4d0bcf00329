"""rotate_kernel bit for bit against the numpy restatement of the randomised block Hadamard rotation
(tests/rotate_cases.py): every block size, both directions, rows around the block and the 4096-parameter tile with
poisoned padding and guards, in place, non-finite and overflowing inputs, the host form, the sign words, and the
rotation composed with the codec's calls around a whole round.  NaN compares as NaN, everything else by its bits."""
from __future__ import annotations

import ctypes
import hashlib

import numpy as np
import pytest

import dp_cases as D
import rotate_cases as R

pytestmark = pytest.mark.gpu

GUARD = np.float32(-123456.75)
FLM_EINVAL = -1   # include/flamingo_hip.h
N_ROWS = 3


@pytest.fixture(scope="module")
def eng():
    from flamingo_amd import MaskEngine
    e = MaskEngine(0)
    yield e
    e.close()


def _signs(L_rot, key=R.KEY):
    import torch
    return torch.from_numpy(R.sign_words(key, L_rot).view(np.int32).copy()).cuda()


def _same(got, want):
    return np.array_equal(R.bits(got), R.bits(want))


def _guards_kept(t, used):
    """every float of the 2-D tensor t behind column `used` still holds GUARD"""
    return bool(np.all(t.cpu().numpy()[:, used:].view(np.uint32) == GUARD.view(np.uint32)))


# ------------------------------------------------------------------ every block size, both directions
@pytest.mark.parametrize("h", R.LOG2_BLOCKS)
def test_rows_match_the_restatement(eng, h):
    import torch
    for L in R.lengths(h):
        L_rot = R.rotated_len(L, h)
        assert eng.rotate_check(L, h) == L_rot
        sb = _signs(L_rot)
        xs = R.rows(N_ROWS, L, 100 * h + L % 97)
        want = np.stack([R.forward(x, R.KEY, h)[0] for x in xs])
        ys = R.rows(N_ROWS, L_rot, 200 * h + L % 89)
        back = np.stack([R.inverse(y, R.KEY, h, L) for y in ys])
        XP, OP = (L + 3) // 4 * 4 + 16, L_rot + 32
        for pad in (np.nan, 1e30):                           # what lies behind L is neither read as input nor counted
            xp = np.full((N_ROWS, XP), pad, np.float32)
            xp[:, :L] = xs
            out = torch.full((N_ROWS, OP), float(GUARD), dtype=torch.float32, device="cuda")
            cnt = torch.full((N_ROWS,), 77, dtype=torch.int32, device="cuda")
            eng.rotate_dev(torch.from_numpy(xp).cuda(), out, L, h, sb, nonfinite=cnt)
            assert _same(out.cpu().numpy()[:, :L_rot], want), (L, pad)
            assert _guards_kept(out, L_rot) and not cnt.cpu().numpy().any(), (L, pad)
        # inverse: L_rot floats in, guards behind the L floats written
        IP, BP = L_rot + 16, (L + 3) // 4 * 4 + 32
        yp = np.full((N_ROWS, IP), np.nan, np.float32)
        yp[:, :L_rot] = ys
        out = torch.full((N_ROWS, BP), float(GUARD), dtype=torch.float32, device="cuda")
        eng.rotate_dev(torch.from_numpy(yp).cuda(), out, L, h, sb, inverse=True)
        assert _same(out.cpu().numpy()[:, :L], back), L
        assert _guards_kept(out, L), L


@pytest.mark.parametrize("h", (4, 8, 12))
def test_in_place(eng, h):
    import torch
    L = 2 * 4096 + (1 << h) // 2 + 3
    L_rot = R.rotated_len(L, h)
    sb = _signs(L_rot)
    xs = R.rows(N_ROWS, L, 31 + h)
    want = np.stack([R.forward(x, R.KEY, h)[0] for x in xs])
    buf = np.full((N_ROWS, L_rot + 8), np.nan, np.float32)
    buf[:, :L] = xs
    t = torch.from_numpy(buf).cuda()
    eng.rotate_dev(t, t, L, h, sb)
    got = t.cpu().numpy()
    assert _same(got[:, :L_rot], want) and np.isnan(got[:, L_rot:]).all()
    # ... and back, in place: the first L floats are rewritten, the rest of the rotated row stays
    back = np.stack([R.inverse(y, R.KEY, h, L) for y in want])
    eng.rotate_dev(t, t, L, h, sb, inverse=True)
    again = t.cpu().numpy()
    assert _same(again[:, :L], back) and _same(again[:, L:L_rot], want[:, L:]) and np.isnan(again[:, L_rot:]).all()
    bound = 2 * (h + 1) * 2.0 ** -24 * np.sqrt((xs.astype(np.float64) ** 2).sum(axis=1).max())   # whole-row norm: loose
    assert np.max(np.abs(back.astype(np.float64) - xs)) <= bound


def test_nonfinite_inputs_are_zeroed_and_counted(eng):
    import torch
    h, H = 6, 64
    L = 2 * H + 10
    L_rot = R.rotated_len(L, h)
    xs = R.rows(N_ROWS, L, 5)
    xs[0, 0], xs[0, H - 1], xs[0, L - 1] = np.nan, np.inf, -np.inf          # a block's first and last parameter, L - 1
    xs[1, H], xs[1, 2 * H - 1] = -np.inf, np.nan
    want = [R.forward(x, R.KEY, h) for x in xs]
    assert [w[1] for w in want] == [3, 2, 0]
    xp = np.full((N_ROWS, L + 2 + 16), np.nan, np.float32)
    xp[:, :L] = xs
    out = torch.zeros((N_ROWS, L_rot), dtype=torch.float32, device="cuda")
    cnt = torch.full((N_ROWS,), 77, dtype=torch.int32, device="cuda")
    eng.rotate_dev(torch.from_numpy(xp).cuda(), out, L, h, _signs(L_rot), nonfinite=cnt)
    assert _same(out.cpu().numpy(), np.stack([w[0] for w in want]))
    assert list(cnt.cpu().numpy()) == [3, 2, 0]
    got, counts = eng.rotate(xs, R.KEY, h, return_nonfinite=True)
    assert _same(got, np.stack([w[0] for w in want])) and list(counts) == [3, 2, 0]
    with pytest.raises(RuntimeError):                                        # the inverse counts nothing
        eng.rotate_dev(out, out, L, h, _signs(L_rot), inverse=True, nonfinite=cnt)


def test_refusals_on_the_device(eng):
    """What flm_rotate and flm_rotate_dev answer to N <= 0, by code and text (tests/test_l2_gpu.py has the calls with
    the clip, which differ).  Every case returns before a launch: one-element arrays and NULL stand in for the rows."""
    import torch
    from flamingo_amd._lib import p_u32
    lib, ctx, stream, L, h = eng.lib, eng.ctx, eng._stream_handle(None), 100, 5
    cnt_host = np.full(1, 77, np.uint32)
    cnt_dev = torch.full((1,), 77, dtype=torch.int32, device="cuda")
    cnt = ctypes.c_void_p(cnt_dev.data_ptr())

    def refused(rc, text):
        return rc == FLM_EINVAL and text in lib.flm_last_error(ctx)

    # N = 0: nothing to do, whatever the arrays; N < 0 is refused
    assert lib.flm_rotate(ctx, None, 0, L, h, None, 0, None, None) == 0
    assert lib.flm_rotate_dev(ctx, None, 0, 0, L, h, None, 0, None, 0, None, stream) == 0
    assert refused(lib.flm_rotate(ctx, None, -1, L, h, None, 0, None, None), b"negative N")
    assert refused(lib.flm_rotate_dev(ctx, None, 0, -1, L, h, None, 0, None, 0, None, stream), b"negative N")
    # counts asked of the inverse: refused before the N = 0 return, and the counts stay as they were
    text = b"the inverse rotation counts nothing: nonfinite must be NULL"
    for N in (0, 1):
        assert refused(lib.flm_rotate(ctx, None, N, L, h, None, 1, None, p_u32(cnt_host)), text)
        assert refused(lib.flm_rotate_dev(ctx, None, 0, N, L, h, None, 1, None, 0, cnt, stream), text)
    # ... while the forward direction at N = 0 takes them and touches nothing
    assert lib.flm_rotate_dev(ctx, None, 0, 0, L, h, None, 0, None, 0, cnt, stream) == 0
    torch.cuda.synchronize()
    assert cnt_host[0] == 77 and int(cnt_dev.cpu()[0]) == 77


@pytest.mark.parametrize("h", (4, 7, 12))
def test_finite_inputs_that_overflow_inside_the_butterflies(eng, h):
    L = (1 << h) + 5
    xs = np.full((2, L), 3e38, np.float32)
    xs[1, ::3] = -3e38
    want = [R.forward(x, R.KEY, h) for x in xs]
    assert all(w[1] == 0 for w in want) and not np.isfinite(want[0][0]).all()
    got, counts = eng.rotate(xs, R.KEY, h, return_nonfinite=True)
    assert _same(got, np.stack([w[0] for w in want])) and not counts.any()
    y = np.stack([w[0] for w in want])
    assert _same(eng.rotate(y, R.KEY, h, inverse=True, L=L), np.stack([R.inverse(r, R.KEY, h, L) for r in y]))


@pytest.mark.parametrize("N", (1, 5))
def test_host_form_equals_device_form(eng, N):
    import torch
    h, L = 9, 4096 + 700
    L_rot = R.rotated_len(L, h)
    xs = R.rows(N, L, 70 + N)
    out = torch.empty((N, L_rot), dtype=torch.float32, device="cuda")
    eng.rotate_dev(torch.from_numpy(xs).cuda(), out, L, h, _signs(L_rot))
    host = eng.rotate(xs, R.KEY, h)
    assert host.shape == (N, L_rot) and host.tobytes() == out.cpu().numpy().tobytes()
    assert _same(host, np.stack([R.forward(x, R.KEY, h)[0] for x in xs]))
    back = torch.empty((N, L), dtype=torch.float32, device="cuda")
    eng.rotate_dev(out, back, L, h, _signs(L_rot), inverse=True)
    assert eng.rotate(host, R.KEY, h, inverse=True, L=L).tobytes() == back.cpu().numpy().tobytes()
    if N == 1:                                               # a vector in, a vector out
        assert eng.rotate(xs[0], R.KEY, h).tobytes() == host[0].tobytes()


def test_sign_words_are_the_prg_of_the_key(eng):
    import torch
    h, L = 5, 100
    L_rot = R.rotated_len(L, h)
    words = -(-L_rot // 32)
    assert np.array_equal(eng.prg_expand([R.KEY], words)[0], R.sign_words(R.KEY, L_rot))
    key = torch.from_numpy(np.frombuffer(R.KEY, np.uint8).reshape(1, 32).copy()).cuda()
    sb = torch.zeros((1, words), dtype=torch.int32, device="cuda")
    eng.prg_expand_dev(key, sb, words)
    assert np.array_equal(sb.cpu().numpy().view(np.uint32)[0], R.sign_words(R.KEY, L_rot))
    xs = R.rows(2, L, 9)
    a, b = eng.rotate(xs, R.KEY, h), eng.rotate(xs, R.KEY2, h)
    assert _same(a, np.stack([R.forward(x, R.KEY, h)[0] for x in xs]))
    assert _same(b, np.stack([R.forward(x, R.KEY2, h)[0] for x in xs])) and a.tobytes() != b.tobytes()


# ------------------------------------------------------------------ composed with the codec around a round
# (call, pack, f, c, stochastic, noise bits): P = 1 at (16, 4); P = 2 at (7, 1), n <= 255; noise at (4, 1, 2, 32)
CHAINS = (("plain", 1, 16, 4.0, False, 0), ("pack", 2, 7, 1.0, False, 0), ("pack", 2, 7, 1.0, True, 0),
          ("noise", 2, 4, 1.0, True, 32))


@pytest.mark.parametrize("h", (5, 12))
def test_rotation_composes_with_the_codec(eng, h):
    n, L = 5, 4096 + 7
    L_rot = R.rotated_len(L, h)
    rng = np.random.default_rng(600 + h)
    xs = (rng.standard_normal((n, L)) * 0.01).astype(np.float32)
    xs[:, rng.choice(L, 16, replace=False)] = 0.75            # a few large coordinates among many small ones
    key = hashlib.sha256(b"chain key %d" % h).digest()
    ys_want = np.stack([R.forward(x, key, h)[0] for x in xs])
    ys = eng.rotate(xs, key, h)
    assert _same(ys, ys_want)
    counts = (1, 2, 0, 3, 1)
    seeds = rng.integers(0, 256, size=(sum(counts), 32), dtype=np.uint8)
    signs = rng.choice(np.array([-1, 1], np.int8), size=sum(counts))
    seg = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    dithers = [hashlib.sha256(b"chain dither %d %d" % (h, i)).digest() for i in range(n)]
    noises = [D.seed(900 + 10 * h + i) for i in range(n)]
    for call, P, f, c, st, b in CHAINS:
        assert D.headroom_ok(f, c, P, b, n)
        d = dithers if st else None
        if call == "plain":
            rows = eng.client_encode_mask(seg, seeds, signs, L_rot, ys, f, c, dither=d)
        elif call == "pack":
            rows = eng.client_encode_pack_mask(seg, seeds, signs, L_rot, ys, f, c, P, dither=d)
        else:
            rows = eng.client_encode_noise_mask(seg, seeds, signs, L_rot, ys, f, c, P, dither=d, noise_bits=b, noise=noises)
        enc = sum(D.encode_any(y, f, c, P, d[i] if d else None, noises[i] if b else None, b)[0].astype(np.uint64)
                  for i, y in enumerate(ys_want)).astype(np.uint32)
        total = eng.aggregate_unmask(rows, seeds, -signs)      # the masks cancel: the sum of the encodings
        assert np.array_equal(total, enc), (call, st)
        mean_rot = eng.decode_sum(total, f, n) if P == 1 else eng.decode_unpack(total, L_rot, f, c, P, n, noise_bits=b)
        want_rot = D.decode_any(enc, L_rot, f, c, P, b, n)
        assert mean_rot.tobytes() == want_rot.tobytes(), (call, st)
        mean = eng.rotate(mean_rot, key, h, inverse=True, L=L)
        assert mean.shape == (L,) and _same(mean, R.inverse(want_rot, key, h, L)), (call, st)


def test_one_hot_claim_through_the_engine(eng):
    c = R.ONE_HOT
    xs = R.one_hot_clients()
    n, L, h, f, clip, P = len(xs), c["L"], c["h"], c["f"], c["c"], c["pack"]
    L_rot = R.rotated_len(L, h)
    exact = (xs.astype(np.float64).sum(axis=0) / n).astype(np.float32)
    seg = np.zeros(n + 1, np.int64)
    none = np.zeros((0, 32), np.uint8)
    ys = eng.rotate(xs, R.KEY, h)
    assert float(np.abs(ys).max()) == 0.125                   # 16 steps of 2^-7, half the clip
    rows, clipped = eng.client_encode_pack_mask(seg, none, [], L_rot, ys, f, clip, P, return_clipped=True)
    assert not clipped.any()
    total = eng.aggregate_unmask(rows, none, [])
    back = eng.rotate(eng.decode_unpack(total, L_rot, f, clip, P, n), R.KEY, h, inverse=True, L=L)
    assert np.all(back == exact)                              # by value: -0.0 occurs
    rows, clipped = eng.client_encode_pack_mask(seg, none, [], L, xs, f, clip, P, return_clipped=True)
    plain = eng.decode_unpack(eng.aggregate_unmask(rows, none, []), L, f, clip, P, n)
    assert list(clipped) == [1] * n and float(exact[5]) - float(plain[5]) == 0.1875
