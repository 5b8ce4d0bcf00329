"""Conditional stochastic rounding's kernels bit for bit against the restatement (tests/round_cases.py): the sums of
squares at rows around the 16-parameter thread, the 4096-parameter tile and many tiles, with NaN in every row's
padding and other values in every output beforehand; the encoder's own words under the chosen seed, unpacked and
packed, which ties the pass to the kernel it steers; the selection at bounds taken from the case's own sums, with guard
words behind every output; the wrap guard; the host form, the stream contract and the binding against the C call."""
from __future__ import annotations

import ctypes

import numpy as np
import pytest

import codec_cases as CC
import pack_cases as PC
import round_cases as RC

pytestmark = pytest.mark.gpu

GUARD64, GUARD32, GUARD8 = -0x0123456789ABCDEF, 0x5A5A1234, 0xA7


@pytest.fixture(scope="module")
def eng():
    from flamingo_amd import MaskEngine
    e = MaskEngine(0)
    yield e
    e.close()


def _padded(xs, pitch, fill=np.nan):
    """the rows at `pitch` floats, `fill` behind each"""
    import torch
    xs = np.asarray(xs, np.float32)
    buf = np.full((xs.shape[0], pitch), fill, np.float32)
    buf[:, :xs.shape[1]] = xs
    return torch.from_numpy(buf).cuda()


def _select(eng, x_dev, L, f, c, cands, max_sumsq, stream=None, sync=True):
    """flm_round_select_dev on the device rows: (sumsq (N, A), dither (N, 32), chosen (N,)) as numpy, from buffers that
    held other values and with guard words behind each, which must come back untouched."""
    import torch
    N, A = cands.shape[:2]
    S = torch.full((N * A + 4,), GUARD64, dtype=torch.int64, device="cuda")
    D = torch.full((N + 2, 32), GUARD8, dtype=torch.uint8, device="cuda")
    ch = torch.full((N + 4,), GUARD32, dtype=torch.int32, device="cuda")
    cd = torch.from_numpy(np.ascontiguousarray(cands)).cuda()
    got = eng.round_select_dev(x_dev, L, f, c, cd, max_sumsq, S, D[:N], ch, stream=stream)
    assert got.data_ptr() == D.data_ptr()
    if not sync:
        return S, D, ch
    torch.cuda.synchronize()
    S, D, ch = S.cpu().numpy(), D.cpu().numpy(), ch.cpu().numpy()
    assert (S[N * A:] == GUARD64).all() and (D[N:] == GUARD8).all() and (ch[N:] == GUARD32).all()
    return S[:N * A].view(np.uint64).reshape(N, A), D[:N], ch[:N].view(np.uint32)


def _pitch(L, extra=16):
    return (L + 3) // 4 * 4 + extra


# ------------------------------------------------------------------ the sums
@pytest.mark.parametrize("L", RC.LENGTHS)
def test_sums_match_the_restatement(eng, L):
    f, c = 7, 1.0
    for N, A in ((1, 8), (3, 3), (3, 1)):
        xs = RC.random_rows(N, L, c, L % 97 + N)
        cands = RC.candidates(f"sums {L}", N, A)
        want = RC.sums(xs, f, c, cands)
        S, D, ch = _select(eng, _padded(xs, _pitch(L)), L, f, c, cands, 2 ** 63)      # pitch > L, NaN behind every row
        assert S.tolist() == want, (L, N, A)
        assert (ch == 0).all() and D.tobytes() == cands[:, 0].tobytes()
    # the last row alone, at another pitch, with other values behind it: the same sums
    S1, _, _ = _select(eng, _padded(xs[-1:], _pitch(L, 64), 1e30), L, f, c, cands[-1:], 0)
    assert S1.tolist() == want[-1:]


def test_sums_of_the_edge_value_and_threshold_rows(eng):
    for name, f, c, x, cands in RC.cases():
        L = len(x)
        for A in RC.ATTEMPTS:
            want = RC.sums([x], f, c, cands[None, :A])
            S, _, _ = _select(eng, _padded(x[None, :], _pitch(L, 4)), L, f, c, cands[None, :A], 0)
            assert S.tolist() == want, (name, A)
    # the threshold row under DITHER and under the two other candidates: three different sums, in the candidates' order
    x, _, cands = RC.threshold_case()
    S, _, _ = _select(eng, _padded(x[None, :], _pitch(len(x))), len(x), CC.THRESHOLD_F, CC.THRESHOLD_C, cands[None], 0)
    assert len(set(S[0].tolist())) == 3 and S[0, 1] == RC.sumsq(x, CC.THRESHOLD_F, CC.THRESHOLD_C, CC.DITHER)


def test_wrap_guard(eng):
    f, c, x, want = RC.WRAP_GUARD
    S, D, ch = _select(eng, _padded(x[None, :], 4), 3, f, c, RC.candidates("wrap", 1, 2), want)
    assert S.tolist() == [[want, want]] and want == 3 * 2 ** 60 and ch[0] == 0
    _, _, ch = _select(eng, _padded(x[None, :], 4), 3, f, c, RC.candidates("wrap", 1, 2), want - 1)
    assert ch[0] == 2


# ------------------------------------------------------------------ the encoder agrees
def _encode_unmasked(eng, x_dev, L, f, c, pack, dither_dev):
    """client_encode[_pack]_mask_dev with no mask seeds for any client: the encoder's own words."""
    import torch
    N = x_dev.shape[0]
    Lw = -(-L // pack)
    out = torch.zeros((N, (Lw + 3) // 4 * 4), dtype=torch.int32, device="cuda")
    seg, signs = np.zeros(N + 1, np.int64), np.zeros(0, np.int8)
    seeds = torch.zeros((0, 32), dtype=torch.uint8, device="cuda")
    if pack == 1:
        eng.client_encode_mask_dev(seg, seeds, signs, out, L, x_dev, f, c, dither_dev=dither_dev)
    else:
        eng.client_encode_pack_mask_dev(seg, seeds, signs, out, L, x_dev, f, c, pack, dither_dev=dither_dev)
    torch.cuda.synchronize()
    return out.cpu().numpy()[:, :Lw].view(np.uint32)


@pytest.mark.parametrize("L", (17, 4097, 8193))
def test_the_encoder_rounds_to_the_sum_the_pass_chose(eng, L):
    import torch
    f, c, N, A = 7, 1.0, 3, 3
    xs = RC.random_rows(N, L, c, 50 + L % 13)
    xs[0, :min(L, len(CC.value_row(f, c)))] = CC.value_row(f, c)[:L]
    cands = RC.candidates(f"agree {L}", N, A)
    want = RC.sums(xs, f, c, cands)
    bound = sorted(v for row in want for v in row)[N * A // 2]                       # some rows pass late or never
    x_dev = _padded(xs, _pitch(L))
    S, D, ch = _select(eng, x_dev, L, f, c, cands, bound)
    assert S.tolist() == want and [RC.select(r, bound) for r in want] == ch.tolist()
    d_dev = torch.from_numpy(D.copy()).cuda()
    words = _encode_unmasked(eng, x_dev, L, f, c, 1, d_dev)
    B = PC.bias(f, c)
    fields = _encode_unmasked(eng, x_dev, L, f, c, 2, d_dev)
    for i in range(N):
        a = int(ch[i]) if ch[i] < A else 0
        assert D[i].tobytes() == cands[i, a].tobytes()
        q1 = words[i].view(np.int32).tolist()
        assert sum(v * v for v in q1) == int(S[i, a]), (L, i)
        u = np.stack([fields[i] & 0xFFFF, fields[i] >> 16], axis=1).reshape(-1)[:L].astype(np.int64)
        assert sum(v * v for v in (u - B).tolist()) == int(S[i, a]), (L, i)
        assert (u - B).tolist() == q1


def test_the_encoder_agrees_at_the_threshold_row(eng):
    import torch
    x, _, cands = RC.threshold_case()
    f, c, L = CC.THRESHOLD_F, CC.THRESHOLD_C, len(x)
    x_dev = _padded(x[None, :], _pitch(L))
    for first in range(3):
        order = np.roll(cands, -first, axis=0)[None]
        S, D, ch = _select(eng, x_dev, L, f, c, order, 2 ** 62)
        assert ch[0] == 0 and D[0].tobytes() == order[0, 0].tobytes()
        words = _encode_unmasked(eng, x_dev, L, f, c, 1, torch.from_numpy(D.copy()).cuda())
        assert sum(v * v for v in words[0].view(np.int32).tolist()) == int(S[0, 0]) == RC.sumsq(x, f, c, bytes(order[0, 0]))


# ------------------------------------------------------------------ the selection
@pytest.mark.parametrize("A", RC.ATTEMPTS)
def test_selection_at_bounds_from_the_cases_own_sums(eng, A):
    f, c, N, L = 7, 1.0, 5, 4097
    xs = RC.random_rows(N, L, c, 77 + A)
    xs[1] *= np.float32(0.25)                                                         # rows of different norms
    xs[3] *= np.float32(0.5)
    cands = RC.candidates(f"select {A}", N, A)
    want = RC.sums(xs, f, c, cands)
    flat = sorted({v for row in want for v in row})
    assert len(flat) >= min(N * A, 5)
    bounds = [flat[0] - 1, flat[0], flat[len(flat) // 2], flat[len(flat) // 2] + 1, flat[-1] - 1, flat[-1], 2 ** 64 - 1]
    bounds += [row[a] for row in want for a in range(A)]                              # equal to a sum: it passes
    x_dev = _padded(xs, _pitch(L))
    seen = set()
    for b in bounds:
        S, D, ch = _select(eng, x_dev, L, f, c, cands, b)
        assert S.tolist() == want
        pick = [RC.select(row, b) for row in want]
        assert ch.tolist() == pick, b
        for i, a in enumerate(pick):
            assert D[i].tobytes() == cands[i, a if a < A else 0].tobytes(), (b, i)
            seen.add("none" if a == A else "first" if a == 0 else "later")
    assert seen == ({"none", "first", "later"} if A > 1 else {"none", "first"})


# ------------------------------------------------------------------ host form, binding, stream
def test_host_form_and_binding_equal_the_device_form(eng):
    f, c, N, A, L = 7, 1.0, 3, 4, 8193
    xs = RC.random_rows(N, L, c, 5)
    cands = RC.candidates("host", N, A)
    want = RC.sums(xs, f, c, cands)
    bound = sorted(v for row in want for v in row)[5]
    S, D, ch = _select(eng, _padded(xs, _pitch(L)), L, f, c, cands, bound)
    # MaskEngine.round_select ...
    d2, ch2, S2 = eng.round_select(xs, f, c, cands, bound)
    assert S2.dtype == np.uint64 and S2.shape == (N, A) and d2.shape == (N, 32) and ch2.dtype == np.uint32
    assert S2.tolist() == want == S.tolist() and d2.tobytes() == D.tobytes() and ch2.tolist() == ch.tolist()
    assert 0 < sum(int(v) for v in ch2) and min(ch2) < A
    # ... against the C call itself, on buffers that held other values
    hs = np.full((N, A), 0xFFFFFFFFFFFFFFFF, np.uint64)
    hd, hc = np.full((N, 32), 0x55, np.uint8), np.full(N, 0xFFFFFFFF, np.uint32)
    x = np.ascontiguousarray(xs, np.float32)
    rc = eng.lib.flm_round_select(eng.ctx, x.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), N, L, f, c,
                                  cands.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)), A, bound,
                                  hs.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)),
                                  hd.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)),
                                  hc.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)))
    assert rc == 0 and hs.tolist() == want and hd.tobytes() == d2.tobytes() and hc.tolist() == ch2.tolist()
    # one row as a vector with a list of seeds
    d1, c1, S1 = eng.round_select(xs[0], f, c, [bytes(k) for k in cands[0]], bound)
    assert S1.tolist() == want[:1] and d1.tobytes() == d2[:1].tobytes() and c1.tolist() == ch2[:1].tolist()
    # round_bound and round_check are the C calls
    assert eng.round_bound(2.28125, 7, 4096, tail=1.0) == RC.bound(2.28125, 7, 4096, 1.0)
    assert eng.round_bound(2.28125, 7, 4096, beta=0.1) == RC.bound(2.28125, 7, 4096, RC.tail_of(0.1))
    eng.round_check(L, f, c, 8)
    for bad in (lambda: eng.round_check(L, f, c, 9), lambda: eng.round_bound(1.0, 7, 16), lambda: eng.round_bound(1.0, 7, 16, 1.0, 0.1),
                lambda: eng.round_select(xs, f, c, cands[:2], bound), lambda: eng.round_select(xs, 31, c, cands, bound)):
        with pytest.raises(RuntimeError):
            bad()


def test_refusals_on_the_device(eng):
    import torch
    L, N, A = 100, 2, 2
    x = torch.zeros((N, 104), dtype=torch.float32, device="cuda")
    cd = torch.zeros((N, A, 32), dtype=torch.uint8, device="cuda")
    S = torch.zeros(N * A, dtype=torch.int64, device="cuda")
    D = torch.zeros((N, 32), dtype=torch.uint8, device="cuda")
    ch = torch.zeros(N, dtype=torch.int32, device="cuda")
    eng.round_select_dev(x, L, 7, 1.0, cd, 0, S, D, ch)
    for call in (lambda: eng.round_select_dev(x[:, 1:], L, 7, 1.0, cd, 0, S, D, ch),          # rows off 16 bytes
                 lambda: eng.round_select_dev(x, L, 7, 1.0, cd, 0, S[:3], D, ch),            # too few sums
                 lambda: eng.round_select_dev(x, L, 7, 1.0, cd[:1], 0, S, D, ch),            # candidates of another N
                 lambda: eng.round_select_dev(x, L, 7, 0.0, cd, 0, S, D, ch),
                 lambda: eng.round_select_dev(x, L, 7, 1.0, cd, 0, S, D, ch[:1])):
        with pytest.raises(RuntimeError):
            call()
    lib, ctx, st = eng.lib, eng.ctx, eng._stream_handle(None)
    p = ctypes.c_void_p(x.data_ptr())
    assert lib.flm_round_select_dev(ctx, None, 0, 0, L, 7, 1.0, None, 1, 0, None, None, None, st) == 0      # N = 0: nothing
    assert lib.flm_round_select_dev(ctx, p, 104, -1, L, 7, 1.0, p, 1, 0, p, p, p, st) == -1
    assert lib.flm_round_select_dev(ctx, p, 104, 1, L, 7, 1.0, p, 1, 0, None, p, p, st) == -1 and b"NULL" in lib.flm_last_error(ctx)
    assert lib.flm_round_select_dev(ctx, p, 102, 1, L, 7, 1.0, p, 1, 0, p, p, p, st) == -1 and b"pitch" in lib.flm_last_error(ctx)
    off = ctypes.c_void_p(x.data_ptr() + 4)
    assert lib.flm_round_select_dev(ctx, p, 104, 1, L, 7, 1.0, p, 1, 0, off, p, p, st) == -1 and b"8-byte" in lib.flm_last_error(ctx)
    torch.cuda.synchronize()


def test_side_stream_then_encode_gives_the_synchronous_bits(eng):
    """The call on a side stream, its dither output handed straight to the encode on that stream, nothing synchronised
    in between: the bits of the synchronous host path."""
    import torch
    f, c, N, A, L = 7, 1.0, 3, 4, 4096 + 11
    xs = RC.random_rows(N, L, c, 9)
    cands = RC.candidates("stream", N, A)
    want = RC.sums(xs, f, c, cands)
    bound = sorted(v for row in want for v in row)[4]
    seeds = [RC.seed("mask", k) for k in range(4)]
    seg, signs = np.array([0, 2, 2, 4], np.int64), np.array([1, -1, -1, 1], np.int8)
    d_host, ch_host, _ = eng.round_select(xs, f, c, cands, bound)
    sync = eng.client_encode_mask(seg, seeds, signs, L, xs, f, c, dither=d_host)
    x_dev = _padded(xs, _pitch(L))
    seeds_dev = torch.from_numpy(np.frombuffer(b"".join(seeds), np.uint8).reshape(4, 32).copy()).cuda()
    out = torch.zeros((N, _pitch(L)), dtype=torch.int32, device="cuda")
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        S, D, ch = _select(eng, x_dev, L, f, c, cands, bound, stream=side, sync=False)
        eng.client_encode_mask_dev(seg, seeds_dev, signs, out, L, x_dev, f, c, dither_dev=D[:N], stream=side)
    side.synchronize()
    assert ch.cpu().numpy()[:N].view(np.uint32).tolist() == ch_host.tolist() == [RC.select(r, bound) for r in want]
    assert D.cpu().numpy()[:N].tobytes() == d_host.tobytes()
    assert out.cpu().numpy()[:, :L].view(np.uint32).tobytes() == sync.tobytes()
