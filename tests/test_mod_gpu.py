"""decode_unpack_mod_kernel on the GPU, bit for bit against tests/mod_cases.py: summed words built from integer field
sums (no encoding needed) over every launch shape, bias regime and edge value, with and without stats, host and device
forms, the padding behind L, the old decode inside the old rule; then whole rounds the worst-case rule refuses, encoded
on the GPU, through the engine and through the store."""
from __future__ import annotations

import importlib.util
import os

import numpy as np
import pytest

import dgauss_cases as G
import dp_cases as D
import mod_cases as MC
import pack_cases as PC

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAD = 24                      # NaN floats behind L that no decode may touch


@pytest.fixture(scope="module")
def eng():
    from flamingo_amd import MaskEngine
    e = MaskEngine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def rounds():
    """The issue's rounds on the CPU, once: ROUNDS[k] -> (Q, S)."""
    return {r: MC.round_case(*r) for r in MC.ROUNDS}


def _dev(eng, S, L, f, c, P, n, b, g, stats=True):
    """The device form on padded tensors -> (floats[L], (near, max) or None, the padding behind L)."""
    import torch
    total = torch.from_numpy(S.view(np.int32)).cuda()
    out = torch.full((L + PAD,), float("nan"), dtype=torch.float32, device="cuda")
    st = torch.full((2,), 0x5A5A5A5A, dtype=torch.int32, device="cuda") if stats else None     # zeroed by the call
    eng.decode_unpack_mod_dev(total, out, L, f, c, P, n, noise_bits=b, guard=g, stats=st)
    torch.cuda.synchronize()
    o = out.cpu().numpy()
    return o[:L], (tuple(int(v) for v in st.cpu().numpy().view(np.uint32)) if stats else None), o[L:]


# ------------------------------------------------------------------ every shape, bias regime and edge value
@pytest.mark.parametrize("P", MC.PACKS)
def test_shapes_biases_and_edges(eng, P):
    H = MC.half(P)
    for L in MC.shapes(P):
        for k, (f, c, b, n) in enumerate(MC.BIAS_CASES):
            bn = D.bias_n(f, c, b)
            g = (1, MC.guard(P, 0.5), H, MC.guard(P, 0.9))[k]
            Q = MC.edge_row(P, g, L)
            S = MC.summed_words(Q, P, n, bn)
            want, qh = MC.decode_mod(S, L, f, P, n, bn)
            assert np.array_equal(qh, Q)
            got, st = eng.decode_unpack_mod(S, L, f, c, P, n, noise_bits=b, guard=g)
            assert got.dtype == np.float32 and got.tobytes() == want.tobytes(), (P, L, f, c, b, n)
            assert st == MC.stats(Q, g), (P, L, g)
            got2, none = eng.decode_unpack_mod(S, L, f, c, P, n, noise_bits=b, guard=g, stats=False)
            assert none is None and got2.tobytes() == want.tobytes()
            d, dst, pad = _dev(eng, S, L, f, c, P, n, b, g)
            assert d.tobytes() == want.tobytes() and dst == st and np.isnan(pad).all()
            d2, none, pad = _dev(eng, S, L, f, c, P, n, b, g, stats=False)
            assert none is None and d2.tobytes() == want.tobytes() and np.isnan(pad).all()


@pytest.mark.parametrize("P", MC.PACKS)
def test_second_grid_stride_trip_and_a_tail(eng, P):
    """L = 4 P 2^20 + 4 P + 3: the 4096 groups take 2^20 quads in their first trip, one more in a second, and three
    parameters are left for the tail; n B_n at or above 2^32."""
    f, c, b, n = MC.BIAS_CASES[2]
    bn, L, g = D.bias_n(f, c, b), MC.long_shape(P), MC.guard(P, 0.75)
    assert L // (4 * P) == 2 ** 20 + 1 and L % (4 * P) == 3 and n * bn >= 2 ** 32
    Q = MC.random_q(P, L, 5 + P)
    e = MC.edge_q(P, g)
    Q[-len(e):] = e                                            # the second trip's quad and the tail hold the edges
    S = MC.summed_words(Q, P, n, bn)
    want, qh = MC.decode_mod(S, L, f, P, n, bn)
    assert np.array_equal(qh, Q)
    got, st, pad = _dev(eng, S, L, f, c, P, n, b, g)
    assert got.tobytes() == want.tobytes() and st == MC.stats(Q, g) and np.isnan(pad).all()


@pytest.mark.parametrize("P", MC.PACKS)
def test_wrapped_fields_decode_as_the_rule_says(eng, P):
    """Property 3 on the GPU: fields beyond [-H, H - 1] come back centred, and hand their k to the field above."""
    f, c, b, n = MC.BIAS_CASES[1]
    bn, g = D.bias_n(f, c, b), MC.guard(P, 0.5)
    words = [q for q, _ in MC.handoff_words(P)]
    Q = np.concatenate([np.array(words, np.int64).reshape(-1), MC.random_q(P, 2077, 3, wrapped=True)])
    S = MC.summed_words(Q, P, n, bn)
    want, qh = MC.decode_mod(S, len(Q), f, P, n, bn)
    for lw, qw in enumerate(words):
        assert list(qh[P * lw: P * lw + P]) == MC.model_word(qw, P)[0]
    got, st = eng.decode_unpack_mod(S, len(Q), f, c, P, n, noise_bits=b, guard=g)
    assert got.tobytes() == want.tobytes() and st == MC.stats(qh, g)


# ------------------------------------------------------------------ inside the old rule, the old decode
def test_inside_the_worst_case_rule_the_old_decode(eng):
    cases = [(f, c, P, 0, n) for f, c, P, n in PC.HEADROOM_EDGES] + [tuple(e) for e in D.HEADROOM_EXAMPLES]
    for f, c, P, b, n in cases:
        bn = D.bias_n(f, c, b)
        u = np.random.default_rng(n).integers(0, n * 2 * bn + 1, size=2077, dtype=np.int64)
        u[:4] = (0, n * 2 * bn, n * bn, n * bn + 1)
        S = PC.pack_fields(u, P)
        old = eng.decode_unpack(S, len(u), f, c, P, n, noise_bits=b)
        new, st = eng.decode_unpack_mod(S, len(u), f, c, P, n, noise_bits=b, guard=MC.half(P))
        assert new.tobytes() == old.tobytes() == D.decode_packed_noised(S, len(u), f, c, P, b, n).tobytes()
        assert st == (0, n * bn)
        with pytest.raises(RuntimeError):                        # one more: the old decode refuses, the new one does not
            eng.decode_unpack(S, len(u), f, c, P, n + 1, noise_bits=b)
        eng.decode_unpack_mod(S, len(u), f, c, P, n + 1, noise_bits=b, guard=1)


# ------------------------------------------------------------------ refusals launch nothing
def test_refusals_leave_the_output_alone(eng):
    import torch
    L, P = 37, 2
    S = MC.summed_words(MC.random_q(P, L, 1), P, 5, 3)
    for kw, msg in ((dict(guard=0), "guard"), (dict(guard=MC.half(P) + 1), "guard"), (dict(guard=-3), "guard"),
                    (dict(count=0), "at least 1"), (dict(count=2 ** 31), "2\\^31 - 1"), (dict(noise_bits=3), "noise_bits"),
                    (dict(frac=15), "carry out")):
        a = dict(frac=0, count=5, noise_bits=4, guard=1)
        a.update(kw)
        with pytest.raises(RuntimeError, match=msg):
            eng.decode_unpack_mod(S, L, a["frac"], 1.0, P, a["count"], noise_bits=a["noise_bits"], guard=a["guard"])
    with pytest.raises(RuntimeError, match="pack"):
        eng.decode_unpack_mod(np.zeros(L, np.uint32), L, 0, 1.0, 1, 5)
    buf = torch.full((64,), float("nan"), dtype=torch.float32, device="cuda")
    with pytest.raises(RuntimeError, match="overlap"):          # out may not alias sum
        eng.decode_unpack_mod_dev(buf.view(torch.int32), buf, 32, 0, 1.0, P, 5, noise_bits=4)
    with pytest.raises(RuntimeError, match="overlap"):
        eng.decode_unpack_mod_dev(buf.view(torch.int32)[16:], buf, 32, 0, 1.0, P, 5, noise_bits=4)
    torch.cuda.synchronize()
    assert torch.isnan(buf).all()
    out, st = eng.decode_unpack_mod(np.zeros(0, np.uint32), 0, 0, 1.0, P, 5, noise_bits=4)      # L = 0: nothing, and zeros
    assert len(out) == 0 and st == (0, 0)


# ------------------------------------------------------------------ whole rounds the worst-case rule refuses
def _encode_round(eng, r, mask_seed):
    """The round's rows from the GPU's encode: client 0 also carries one mask, which the server takes off again."""
    f, c, P, rounding, n, L, noise = r
    xs, dithers, noises = MC.round_inputs(c, rounding, n, L, noise)
    seg = np.concatenate([[0], np.ones(n, np.int64)]).astype(np.int64)       # one seed, client 0's
    if noise is not None and noise[0] == "table":
        return eng.client_encode_gauss_mask(seg, [mask_seed], [1], L, xs, f, c, G.real_table(noise[1], noise[2]), noises,
                                            pack=P, dither=dithers)
    return eng.client_encode_noise_mask(seg, [mask_seed], [1], L, xs, f, c, P, dither=dithers,
                                        noise_bits=noise[1] if noise else 0, noise=noises)


@pytest.mark.parametrize("k", range(len(MC.ROUNDS)))
def test_whole_round_beyond_the_worst_case_rule(eng, rounds, k):
    r = MC.ROUNDS[k]
    f, c, P, rounding, n, L, noise = r
    Q, S = rounds[r]
    b, H, M = MC.round_noise_bits(noise), MC.half(P), MC.modulus(P)
    bn = D.bias_n(f, c, b)
    # the premises: the parent's decode refuses the cohort, a carry crosses fields, and no sum wraps
    with pytest.raises(RuntimeError, match="carry out|headroom"):
        eng.decode_unpack(S, L, f, c, P, n, noise_bits=b)
    assert not D.headroom_ok(f, c, P, b, n) and n * bn >= M and int((Q + n * bn).max()) >= M
    assert int(np.abs(Q).max()) < H
    assert (int(np.abs(Q).max()), H, n * bn) == ((4508, 32768, 76800), (50, 128, 400), (938, 32768, 72000), (921, 32768, 68200))[k]
    mask_seed = D.seed(777)
    rows = _encode_round(eng, r, mask_seed)
    total = eng.aggregate_unmask(rows, [mask_seed], [-1])
    assert np.array_equal(total, S)
    g = MC.guard(P, 0.5)
    want, qh = MC.decode_mod(S, L, f, P, n, bn)
    assert np.array_equal(qh, Q)
    got, st = eng.decode_unpack_mod(total, L, f, c, P, n, noise_bits=b, guard=g)
    assert got.tobytes() == want.tobytes() and st == MC.stats(Q, g) == (0, int(np.abs(Q).max()))
    assert got.tobytes() == (Q / (float(n) * 2.0 ** f)).astype(np.float32).tobytes()


def test_store_form_gives_the_engine_calls_floats_and_stats(eng, rounds):
    from flamingo_amd.ingest import VectorStore
    r = MC.ROUNDS[1]
    f, c, P, rounding, n, L, noise = r
    Q, S = rounds[r]
    mask_seed = D.seed(778)
    rows = _encode_round(eng, r, mask_seed)
    g = MC.guard(P, 0.25)
    want, st_want = eng.decode_unpack_mod(S, L, f, c, P, n, guard=g)
    assert st_want == MC.stats(Q, g) and st_want[0] > 0
    st = VectorStore(eng, -(-L // P), n)
    for i in range(n):
        st.add(i, rows[i])
    st.partial_sum()
    st.wait_partial()
    with pytest.raises(RuntimeError):                            # the worst-case form refuses this cohort
        st.unmask_unpack_f32([mask_seed], [-1], L, f, c, P, n)
    got, stats = st.unmask_unpack_mod_f32([mask_seed], [-1], L, f, c, P, n, guard=g)
    assert got.dtype == np.float32 and got.tobytes() == want.tobytes() == MC.decode_mod(S, L, f, P, n, PC.bias(f, c))[0].tobytes()
    assert stats == st_want
    got, none = st.unmask_unpack_mod_f32([mask_seed], [-1], L, f, c, P, n, guard=g, stats=False)      # no counts asked for
    assert none is None and got.tobytes() == want.tobytes()
    with pytest.raises(RuntimeError, match="guard"):
        st.unmask_unpack_mod_f32([mask_seed], [-1], L, f, c, P, n, guard=MC.half(P) + 1)
    with pytest.raises(RuntimeError, match="length"):
        st.unmask_unpack_mod_f32([mask_seed], [-1], L + P, f, c, P, n, guard=g)
    st.close()


# ------------------------------------------------------------------ the reference-side binding
def test_reference_side_binding(eng, monkeypatch, rounds):
    """integration/util_flm.py's modular calls, once each, against the restatement."""
    monkeypatch.setenv("FLM_LIB", os.path.join(ROOT, "flamingo_amd", "lib", "libflamingo_hip.so"))
    import torch  # noqa: F401  (one HIP runtime per process: torch's, loaded first)
    spec = importlib.util.spec_from_file_location("util_flm", os.path.join(ROOT, "integration", "util_flm.py"))
    flm = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(flm)
    r = MC.ROUNDS[0]
    f, c, P, rounding, n, L, noise = r
    Q, S = rounds[r]
    flm.codec_check_modular(f, c, P, 0, n)
    with pytest.raises(RuntimeError):
        flm.codec_check_packed(f, c, P, n)
    with pytest.raises(RuntimeError):
        flm.codec_check_modular(f, c, 4, 0, n)
    g = MC.guard(P, 0.1)
    want = MC.decode_mod(S, L, f, P, n, PC.bias(f, c))[0]
    got, st = flm.decode_unpack_mod(S, L, f, c, P, n, guard=g)
    assert got.tobytes() == want.tobytes() and st == MC.stats(Q, g)
    store = flm.VectorStore(-(-L // P), 2)
    store.add(0, S)
    store.add(1, np.zeros_like(S))
    store.partial()
    got, st = store.unmask_unpack_mod_f32([D.seed(5), D.seed(5)], [1, -1], L, f, c, P, n, guard=g)     # masks that cancel
    assert got.tobytes() == want.tobytes() and st == MC.stats(Q, g)
    store.close()
