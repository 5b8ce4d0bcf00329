"""The decode modulo the field without a GPU: the numpy restatement (tests/mod_cases.py) against its big-integer models
over the rule's three properties, the stats, flm_codec_check_modular through the library for every refusal,
flamingo_amd/modular.py and configure(modular=...)'s rules."""
from __future__ import annotations

import ctypes
import math

import numpy as np
import pytest

import dp_cases as D
import mod_cases as MC
import pack_cases as PC

FLM_EINVAL, FLM_ERANGE = -1, -4     # include/flamingo_hip.h


@pytest.fixture(scope="module")
def lib():
    from flamingo_amd import build, _lib
    build.build()
    return _lib.load()


# ------------------------------------------------------------------ property 1: in range, Qh = Q whatever n B_n is
@pytest.mark.parametrize("pack", MC.PACKS)
def test_in_range_sums_come_back_whatever_the_bias(pack):
    H, M = MC.half(pack), MC.modulus(pack)
    rng = np.random.default_rng(pack)
    g = MC.guard(pack, 0.5)
    for f, c, b, n in MC.BIAS_CASES:
        assert MC.admitted(f, c, pack, b, n)
        bn = D.bias_n(f, c, b)
        for Q in (MC.edge_row(pack, g, 2077), MC.random_q(pack, 5000, 17 * n % 1000)):
            S = MC.summed_words(Q, pack, n, bn)
            out, qh = MC.decode_mod(S, len(Q), f, pack, n, bn)
            assert np.array_equal(qh, Q)
            assert out.dtype == np.float32 and np.array_equal(out, (Q / (float(n) * 2.0 ** f)).astype(np.float32))
            for lw in rng.integers(0, len(Q) // pack, size=200):      # the same in Python integers, word by word
                qw = [int(v) for v in Q[pack * lw: pack * lw + pack]]
                assert MC.word_of(qw, pack, n, bn) == int(S[lw])
                assert MC.rule_word(int(S[lw]), pack, n, bn) == qw == MC.model_word(qw, pack)[0]
    # the premises of the bias cases: below M, at or above M (a carry), at or above 2^32
    nb = [n * D.bias_n(f, c, b) for f, c, b, n in MC.BIAS_CASES]
    assert nb[0] < M and M <= nb[1] < 2 ** 32 and nb[2] >= 2 ** 32 and nb[3] >= 2 ** 32
    assert set(MC.edge_q(pack, g)) <= set(MC.edge_row(pack, g, 2077).tolist()) and -H in MC.edge_q(pack, g)


def test_random_cases_against_the_big_integer_model():
    """40,000 random words: in-range ones (property 1) and wrapped ones (property 3), any admitted (n, B_n)."""
    rng = np.random.default_rng(2021)
    for pack in MC.PACKS:
        H, M = MC.half(pack), MC.modulus(pack)
        for wrapped in (False, True):
            for _ in range(100):
                n = int(rng.choice([1, 2, 255, 4096, 2 ** 20, MC.MAX_COUNT, int(rng.integers(1, MC.MAX_COUNT))]))
                bn = int(rng.integers(1, (M - 1) // 2 + 1))
                Q = MC.random_q(pack, 100 * pack, int(rng.integers(1 << 30)), wrapped)
                S = MC.summed_words(Q, pack, n, bn)
                _, qh = MC.decode_mod(S, len(Q), 3, pack, n, bn)
                for lw in range(100):
                    qw = [int(v) for v in Q[pack * lw: pack * lw + pack]]
                    want, ks = MC.model_word(qw, pack)
                    assert list(qh[pack * lw: pack * lw + pack]) == want == MC.rule_word(int(S[lw]), pack, n, bn)
                    assert all(-H <= v < H for v in want)
                    if not wrapped:
                        assert want == qw and not any(ks)


# ------------------------------------------------------------------ property 3: a wrap is defined
@pytest.mark.parametrize("pack", MC.PACKS)
def test_a_wrapped_field_is_off_by_m_and_hands_k_up(pack):
    H, M = MC.half(pack), MC.modulus(pack)
    seen = set()
    for qw, k in MC.handoff_words(pack):
        want, ks = MC.model_word(qw, pack)
        assert ks[0] == k and (qw[0] - want[0]) == k * M            # off by a multiple of M
        seen.add(k)
        for f, c, b, n in MC.BIAS_CASES:
            bn = D.bias_n(f, c, b)
            S = MC.summed_words(np.array(qw), pack, n, bn)
            out, qh = MC.decode_mod(S, pack, f, pack, n, bn)
            assert list(qh) == want
            if qw[1] + k in range(-H, H):
                assert qh[1] == qw[1] + k                           # the neighbour takes k units of 2^-f / n
                assert out[1] == np.float32((qw[1] + k) / (float(n) * 2.0 ** f))
    assert seen == {1, -1, 2, -2}
    # the hand-off that wraps the field above in turn: H - 1 + 1 -> -H, and 1 goes further up (or out of the word)
    want, ks = MC.model_word([M + 3, H - 1] + [0] * (pack - 2), pack)
    assert want[:2] == [3, -H] and ks[:2] == [1, 1]
    # the sum cannot reveal a wrap: the wrapped word is the word of the in-range values it decodes to
    qw = [H + 9] + [0] * (pack - 1)
    assert MC.word_of(qw, pack, 7, 3) == MC.word_of(MC.model_word(qw, pack)[0], pack, 7, 3)


# ------------------------------------------------------------------ property 2: inside the old rule, the old decode
def test_inside_the_worst_case_rule_the_output_is_the_old_decode():
    cases = [(f, c, P, 0, n) for f, c, P, n in PC.HEADROOM_EDGES] + [tuple(e) for e in D.HEADROOM_EXAMPLES]
    for f, c, P, b, n_max in cases:
        bn = D.bias_n(f, c, b)
        for n in sorted({1, 3, n_max // 2, n_max}):
            assert D.headroom_ok(f, c, P, b, n) and MC.admitted(f, c, P, b, n)
            top = n * 2 * bn                                         # fields of a real sum lie in [0, n 2 B_n]
            rng = np.random.default_rng(n)
            u = rng.integers(0, top + 1, size=4096, dtype=np.int64)
            u[:6] = (0, top, top, 0, n * bn, n * bn + 1)
            S = PC.pack_fields(u, P)
            old = D.decode_packed_noised(S, len(u), f, c, P, b, n)
            new, qh = MC.decode_mod(S, len(u), f, P, n, bn)
            assert new.tobytes() == old.tobytes() and np.array_equal(qh, u - n * bn)
        assert not D.headroom_ok(f, c, P, b, n_max + 1) and MC.admitted(f, c, P, b, n_max + 1)
    # pack_cases.DECODE_WORDS at its own counts: adjacent fields at 0 and at 2^W - 1.  Inside the rule a field holds at
    # most n 2 B <= 2^W - 1, so the words whose fields the count admits decode alike; a field beyond n 2 B is no sum of
    # n contributors, and there the new decode is its centred reading
    for P in PC.PACKS:
        f, c = PC.pack_params(P)
        B, W = PC.bias(f, c), 32 // P
        for n in PC.decode_counts(P):
            S = PC.DECODE_WORDS
            L = len(S) * P
            old = PC.decode_packed(S, L, f, c, P, n)
            new, qh = MC.decode_mod(S, L, f, P, n, B)
            fields = ((S.astype(np.int64)[:, None] >> (W * np.arange(P))) & (2 ** W - 1))
            real = np.repeat((fields <= n * 2 * B).all(axis=1), P)   # whole words of admissible fields
            assert real.any() and new[real].tobytes() == old[real].tobytes()
            assert np.array_equal(qh[real], fields.reshape(-1)[real] - n * B)
            for lw, s in enumerate(S):                               # every word, admissible or not: the rule's reading
                assert list(qh[P * lw: P * lw + P]) == MC.rule_word(int(s), P, n, B)


# ------------------------------------------------------------------ the stats
@pytest.mark.parametrize("pack", MC.PACKS)
def test_stats_count_the_guard_and_take_the_maximum(pack):
    H = MC.half(pack)
    for g in (1, MC.guard(pack, 0.5), H):
        q = np.array([g - 1, g, -g, -(g - 1), 0], np.int64)
        q = q[(q >= -H) & (q < H)]
        near, most = MC.stats(q, g)
        assert near == int((np.abs(q) >= g).sum()) and most == int(np.abs(q).max())
    assert MC.stats(np.array([-H, H - 1]), H) == (1, H)              # Qh = -H counts as H
    assert MC.stats(np.array([H - 1, 1 - H]), H) == (0, H - 1)
    assert MC.stats(np.zeros(0, np.int64), 1) == (0, 0)
    e = MC.edge_row(pack, MC.guard(pack, 0.5), 2077)
    near, most = MC.stats(e, MC.guard(pack, 0.5))
    assert most == H and 0 < near < len(e)


# ------------------------------------------------------------------ the admission, through the library
def test_codec_check_modular_refusals(lib):
    ck = lib.flm_codec_check_modular
    for pack in (0, 1, 3, 8, -2):
        assert ck(4, 1.0, pack, 0, 1) == FLM_EINVAL and lib.flm_last_error(None) == b"pack must be 2 or 4", pack
    for b in (-2, 1, 31, 1026):
        assert ck(4, 1.0, 2, b, 1) == FLM_EINVAL and b"noise_bits" in lib.flm_last_error(None), b
    for f in (-1, 31):
        assert ck(f, 1.0, 2, 0, 1) == FLM_EINVAL and b"frac_bits" in lib.flm_last_error(None)
    for c in (0.0, -1.0, math.inf, math.nan):
        assert ck(4, c, 2, 0, 1) == FLM_EINVAL and b"clip" in lib.flm_last_error(None)
    for n in (0, -1, -2 ** 40):
        assert ck(4, 1.0, 2, 0, n) == FLM_EINVAL and b"at least 1" in lib.flm_last_error(None)
    # one contributor's field does not fit: the packed rule at n = 1
    assert ck(7, 1.0, 4, 0, 1) == FLM_ERANGE and ck(6, 1.9, 4, 12, 1) == FLM_ERANGE and ck(6, 1.9, 4, 10, 1) == 0
    assert ck(15, 1.0, 2, 0, 1) == FLM_ERANGE and ck(14, 1.0, 2, 1024, 1) == 0 and ck(30, 2.0, 2, 0, 1) == FLM_ERANGE
    assert ck(2, 1.0, 4, 246, 1) == 0 and ck(2, 1.0, 4, 248, 1) == FLM_ERANGE          # B_n = 127, 128
    # the count
    assert ck(0, 1.0, 4, 4, MC.MAX_COUNT) == 0 and ck(0, 1.0, 4, 4, MC.MAX_COUNT + 1) == FLM_ERANGE
    assert b"2^31 - 1" in lib.flm_last_error(None)
    assert ck(0, 1.0, 4, 4, 2 ** 62) == FLM_ERANGE


def test_codec_check_modular_admits_what_the_worst_case_refuses(lib):
    ck = lib.flm_codec_check_modular
    for f, c, P, n in PC.HEADROOM_EDGES:
        assert lib.flm_codec_check_packed(f, c, P, n + 1) == FLM_ERANGE and ck(f, c, P, 0, n + 1) == 0 == ck(f, c, P, 0, 4096)
    for f, c, P, b, n in D.HEADROOM_EXAMPLES:
        assert lib.flm_codec_check_noise(f, c, P, b, n + 1, 0) == FLM_ERANGE and ck(f, c, P, b, n + 1) == 0
    assert ck(*D.NO_ROOM[:3], 2, D.NO_ROOM[3]) == 0                  # (7, 1, 2) at n = 255 takes noise now
    assert ck(4, 1.0, 2, 64, 4096) == 0                               # --dp_gauss 3.2 (tail 32) at the headline cohort
    for f, c, P, mode, n, L, noise in MC.ROUNDS:
        b = MC.round_noise_bits(noise)
        assert lib.flm_codec_check_noise(f, c, P, b, n, L) == FLM_ERANGE and ck(f, c, P, b, n) == 0
        assert MC.admitted(f, c, P, b, n) and not D.headroom_ok(f, c, P, b, n)


def test_entry_points_reject_null_handles_and_name_the_feature(lib):
    w = (ctypes.c_uint32 * 4)()
    x = (ctypes.c_float * 4)()
    st = (ctypes.c_uint32 * 2)()
    assert lib.flm_decode_unpack_mod(None, w, 4, 7, 1.0, 2, 0, 1, 1, x, st) == FLM_EINVAL and b"NULL" in lib.flm_last_error(None)
    assert lib.flm_decode_unpack_mod_dev(None, None, 4, 7, 1.0, 2, 0, 1, 1, None, None, None) == FLM_EINVAL
    # the store form checks its rule before it looks at the store: the admission, then the guard, then L
    sm = lib.flm_store_unmask_unpack_mod_f32
    assert sm(None, None, None, 0, 4, 7, 1.0, 3, 0, 1, 1, x, st) == FLM_EINVAL and b"pack" in lib.flm_last_error(None)
    assert sm(None, None, None, 0, 4, 7, 1.0, 4, 0, 1, 1, x, st) == FLM_ERANGE
    for pack, g in ((2, 0), (2, 32769), (4, 129), (2, -1)):
        assert sm(None, None, None, 0, 4, 2, 1.0, pack, 0, 1, g, x, st) == FLM_EINVAL and b"guard" in lib.flm_last_error(None)
    assert sm(None, None, None, 0, 2 ** 32, 2, 1.0, 2, 0, 1, 1, x, st) == FLM_ERANGE
    assert sm(None, None, None, 0, 4, 2, 1.0, 2, 0, 1, 32768, x, st) == FLM_EINVAL and b"bad argument" in lib.flm_last_error(None)
    assert b"modular" in lib.flm_version() and b"dp_gauss" in lib.flm_version()
    from flamingo_amd.engine import MaskEngine
    from flamingo_amd.ingest import VectorStore
    for fn in ("codec_check_modular", "decode_unpack_mod", "decode_unpack_mod_dev"):
        assert callable(getattr(MaskEngine, fn))
    assert callable(VectorStore.unmask_unpack_mod_f32)


# ------------------------------------------------------------------ flamingo_amd/modular.py
def test_modular_guard_and_margin():
    from flamingo_amd import dgauss, modular
    assert modular.half_modulus(2) == 32768 == MC.half(2) and modular.half_modulus(4) == 128 == MC.half(4)
    for pack in (1, 3, 8):
        with pytest.raises(ValueError):
            modular.half_modulus(pack)
    assert modular.guard(2, 0.5) == 16384 and modular.guard(4, 0.5) == 64 and modular.guard(2, 1.0) == 32768
    assert modular.guard(4, 0.3) == 39 and modular.guard(4, 1e-9) == 1 and modular.guard(4, 0.0) == 1      # ceil, then 1..H
    assert modular.guard(4, 7.0) == 128 and modular.guard(2, -1.0) == 1
    for pack in MC.PACKS:
        for fr in (0.001, 0.25, 0.5, 0.75, 0.999, 1.0):
            assert modular.guard(pack, fr) == MC.guard(pack, fr)
    with pytest.raises(ValueError):
        modular.guard(2, math.nan)
    # the issue's example: 1500 clients of the sigma = 3.2 table, max |sum| 938
    var = dgauss.moments(dgauss.table(3.2, 32))[1]
    m = modular.margin_sigmas(2, 1500, 938, var)
    assert m == pytest.approx((32768 - 938) / math.sqrt(1500 * float(var)), rel=1e-12) and 250 < m < 260
    assert modular.margin_sigmas(2, 2200, 921, 30 / 4) == pytest.approx((32768 - 921) / math.sqrt(2200 * 7.5), rel=1e-12)
    assert modular.margin_sigmas(4, 100, 50, 0) == math.inf and modular.margin_sigmas(4, 100, 200, 0) == -math.inf
    assert modular.margin_sigmas(4, 100, 200, 1.0) < 0
    for bad in ((2, 0, 1, 1.0), (2, 1.5, 1, 1.0), (2, 1, 1, -1.0), (2, 1, 1, math.nan), (3, 1, 1, 1.0)):
        with pytest.raises(ValueError):
            modular.margin_sigmas(*bad)


# ------------------------------------------------------------------ the agents' configuration
def test_configure_modular_rules():
    from flamingo_amd.abides.flamingo import protocol as param
    from flamingo_amd.abides import config_flamingo
    param.configure(codec=False)
    try:
        assert param.modular() is None
        with pytest.raises(ValueError, match="packed"):
            param.configure(modular=0.5)                                     # without the codec
        param.configure(codec=(9, 1.0, "stochastic"))
        with pytest.raises(ValueError, match="packed"):
            param.configure(modular=0.5)                                     # unpacked
        param.configure(modular=0)                                           # off stays off anywhere
        param.configure(codec=(9, 1.0, "stochastic", 2))
        for bad in (1.5, -0.1, math.nan, math.inf):
            with pytest.raises(ValueError, match="fraction"):
                param.configure(modular=bad)
        assert param.modular() is None
        param.configure(modular=0.5)
        assert param.modular() == 0.5 and param.modular_guard() == 16384
        param.configure()                                                    # None leaves it as it is
        assert param.modular() == 0.5
        param.configure(modular=1.0)
        assert param.modular_guard() == 32768
        param.configure(codec=(2, 1.0, "nearest", 4), modular=0.25)
        assert param.modular() == 0.25 and param.modular_guard() == 32
        for off in (0, 0.0, False):
            param.configure(modular=0.5)
            param.configure(modular=off)
            assert param.modular() is None
        param.configure(modular=0.5)
        param.configure(codec=False)                                         # what it stands on turned off
        assert param.modular() is None
        param.configure(codec=(9, 1.0, "stochastic", 2))
        assert param.modular() is None                                       # ... and it stays off
    finally:
        param.configure(codec=False)
    _, args = config_flamingo.parse(["-c", "flamingo", "--modular", "0.5"])
    assert args.modular == 0.5 and config_flamingo.parse(["-c", "flamingo"])[1].modular == 0.0


# ------------------------------------------------------------------ the agents, on an engine stand-in
def test_agents_take_the_modular_forms_only_when_asked(monkeypatch, capsys):
    """--float_inputs 9,1,sr,pack2 at n = 64: 64 x 2 x 512 = 65536 > 65535, so the run is refused at set-up as before
    without --modular; with it the server asks codec_check_modular, decodes through the _mod form of the store's method
    and keeps (near, max |Qh|); final_mean is the restatement's decode of the sum of the clients' packed rows."""
    from flamingo_amd.abides.flamingo import protocol
    from test_codec_protocol_cpu import _run
    from test_dp_protocol_cpu import DET, DpEngine, DpStore, _fixture
    from test_pack_protocol_cpu import argv

    class ModStore(DpStore):
        def unmask_unpack_mod_f32(self, seeds, signs, L_params, frac_bits, clip, pack, count=1, noise_bits=0, guard=1):
            out, qh = MC.decode_mod(self.unmask(seeds, signs), L_params, frac_bits, pack, count, D.bias_n(frac_bits, clip, noise_bits))
            return out, MC.stats(qh, guard)

    class ModEngine(DpEngine):
        def vector_store(self, L, capacity):
            return ModStore(L)

        def codec_check_modular(self, frac_bits, clip, n_clients=1, pack=2, noise_bits=0):
            self.calls.append(("codec_check_modular", n_clients))
            if not MC.admitted(frac_bits, clip, pack, noise_bits, n_clients):
                raise RuntimeError("flm_codec_check_modular: refused (code -4)")

    engine = ModEngine()
    sent, drew = _fixture(monkeypatch, engine)
    f, c, P, n = 9, 1.0, 2, 64
    base = argv(n) + DET + ["--float_inputs", "9,1,sr,pack2"]
    try:
        with pytest.raises(RuntimeError, match="code -4"):
            _run(base)
        assert not sent and not any(name == "codec_check_modular" for name, _ in engine.calls)
        with pytest.raises(ValueError, match="packed"):
            _run(argv(n) + DET + ["--float_inputs", "9,1,sr", "--modular", "0.5"])
        res = _run(base + ["--modular", "0.5"])
        assert ("codec_check_modular", n) in engine.calls and protocol.modular() == 0.5
        srv, clients = res["server"], res["clients"]
        H, B = MC.half(P), PC.bias(f, c)
        for it in sorted(srv.means):
            ids = srv.online_ids[it]
            assert len(ids) == n and not PC.headroom_ok(f, c, P, n)
            xs = [np.asarray(clients[i].input_vector, np.float32) for i in ids]
            enc = sum(PC.encode_packed(x, f, c, P, drew[(i, it)][0])[0].astype(np.uint64) for i, x in zip(ids, xs))
            S = (enc & 0xFFFFFFFF).astype(np.uint32)
            assert np.array_equal(srv.results[it], S)
            want, qh = MC.decode_mod(S, len(xs[0]), f, P, n, B)
            assert srv.means[it].tobytes() == want.tobytes() and srv.near_wrap[it] == MC.stats(qh, H // 2)
            assert 0 < srv.near_wrap[it][1] < H
        assert sorted(srv.near_wrap) == sorted(srv.means) and len(srv.means) >= 1
        out = capsys.readouterr().out
        assert out.count(f"decoded modulo the field: H = {H}, guard = {H // 2}, ") == len(srv.means)
    finally:
        from flamingo_amd import params
        protocol.configure(L=params.vector_len, committee=60, codec=False)
