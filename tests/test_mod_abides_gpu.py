"""The agents' --modular option on the GPU: n = 128 clients, 1001 parameters, two iterations, at cohorts the worst-case
headroom rule refuses.  Replayed on the CPU from the dither and noise seeds the clients recorded: final_mean is the
restatement's decode modulo the field (tests/mod_cases.py) of the sum of the online clients' packed rows, bit for bit, and
the server's (near, max |Qh|) are the restatement's stats of the replayed signed sums.  The runs take the deterministic
latency model, under which every client's VECTOR arrives in time: the premises below are about n = 128 exactly."""
import numpy as np
import pytest

import codec_cases as K
import dgauss_cases as G
import l2_cases as l2
import mod_cases as MC
import pack_cases as PC
import rotate_cases as R

pytestmark = pytest.mark.gpu

N, L, P = 128, 1001, 2
FRACTION = 0.5


def _run(monkeypatch, extra):
    from flamingo_amd.abides.config_flamingo import run
    from flamingo_amd.abides.flamingo import protocol
    from flamingo_amd.abides.flamingo.client_agent import SA_ClientAgent
    drew = {}    # (client, iteration) -> (dither seed, noise seed)
    vectors = SA_ClientAgent.sendVectors

    def send_vectors(self, *a, **kw):
        out = vectors(self, *a, **kw)
        drew[(self.id, self.current_iteration)] = (self.dither_seed, self.noise_seed)
        return out

    with monkeypatch.context() as m:
        m.setattr(SA_ClientAgent, "sendVectors", send_vectors)
        try:
            res = run(["-c", "flamingo", "-n", str(N), "-i", "2", "-s", "11", "-k", "--committee_size", "9",
                       "--vector_len", str(L), "--latency", "deterministic"] + extra)
            state = (protocol.modular(), protocol.modular_guard() if protocol.modular() is not None else None,
                     protocol.rotated_len(), protocol.ring_len())
            table = protocol.dp_gauss_table()
            keys = {it: protocol.rotation_key(it) for it in (1, 2)}
        finally:
            protocol.configure(codec=False)
    return res["server"], res["clients"], drew, state, table, keys


def test_modular_admits_the_cohort_the_worst_case_rule_refuses(monkeypatch, capsys):
    """--float_inputs 9,1,sr,pack2: B = 512, so the worst-case rule admits n <= 63 and the run raises without --modular;
    n B = 2^16 at n = 128, so every field's bias carries into the field above it."""
    f, c = 9, 1.0
    B, H, M = PC.bias(f, c), MC.half(P), MC.modulus(P)
    assert B == 512 and (M - 1) // (2 * B) == 63 and not PC.headroom_ok(f, c, P, N) and MC.admitted(f, c, P, 0, N)
    base = ["--float_inputs", "9,1,sr,pack2"]
    with pytest.raises(RuntimeError, match=r"flm_codec_check_noise.*code -4"):
        _run(monkeypatch, base)
    capsys.readouterr()
    srv, clients, drew, state, table, keys = _run(monkeypatch, base + ["--modular", str(FRACTION)])
    assert state == (FRACTION, H // 2, L, -(-L // P)) and table is None
    for it in (1, 2):
        ids = srv.online_ids[it]
        n = len(ids)
        assert n == srv.online_counts[it] == N                       # the deterministic latency model loses no VECTOR
        xs = [np.asarray(clients[i].input_vector, np.float32) for i in ids]
        assert all(len(drew[(i, it)][0]) == 32 and drew[(i, it)][1] is None for i in ids)
        Q = sum(K.encode(x, f, c, drew[(i, it)][0])[0].view(np.int32).astype(np.int64) for i, x in zip(ids, xs))
        enc = sum(PC.encode_packed(x, f, c, P, drew[(i, it)][0])[0].astype(np.uint64) for i, x in zip(ids, xs))
        S = (enc & 0xFFFFFFFF).astype(np.uint32)
        assert np.array_equal(srv.results[it], S)
        # the premises: a carry crosses fields, and no sum wraps (deviation clip / 8: max |Q| near 3 * 10^3)
        assert n * B >= M and int((Q + n * B).max()) >= M and int(np.abs(Q).max()) < H
        assert 10 ** 3 < int(np.abs(Q).max()) < 10 ** 4
        want, qh = MC.decode_mod(S, L, f, P, n, B)
        assert np.array_equal(qh, Q)
        assert srv.means[it].dtype == np.float32 and srv.means[it].tobytes() == want.tobytes()
        assert srv.near_wrap[it] == MC.stats(Q, H // 2) == (0, int(np.abs(Q).max()))
    out = capsys.readouterr().out
    assert out.count(f"decoded modulo the field: H = {H}, guard = {H // 2}, 0 sums at or beyond the guard, max |Qh| = ") == 2
    assert out.count("noise standard deviations (no probability)") == 2


def test_modular_with_the_whole_dp_pipeline(monkeypatch, capsys):
    """--float_inputs 8,1,sr,pack2 --rotate 5 --l2_clip 2.28125 --round_bound 1 --dp_gauss 3.2: B_n = 256 + 32 = 288, so
    the worst-case rule admits n <= 113; replayed as tests/test_dgauss_abides_gpu.py replays its run."""
    from flamingo_amd import dgauss
    f, c, h, norm, sigma, tau, l_rot = 8, 1.0, 5, 2.28125, 3.2, 32, 1024
    Bn, H, M = G.bias_n(f, c, tau), MC.half(P), MC.modulus(P)
    assert Bn == 288 and (M - 1) // (2 * Bn) == 113 and not G.headroom_ok(f, c, P, tau, N) and MC.admitted(f, c, P, 2 * tau, N)
    base = ["--float_inputs", "8,1,sr,pack2", "--rotate", str(h), "--l2_clip", str(norm), "--round_bound", "1",
            "--dp_gauss", str(sigma)]
    with pytest.raises(RuntimeError, match=r"flm_codec_check_gauss.*code -4"):
        _run(monkeypatch, base)
    capsys.readouterr()
    srv, clients, drew, state, table, keys = _run(monkeypatch, base + ["--modular", str(FRACTION)])
    assert state == (FRACTION, H // 2, l_rot, l_rot // P)
    cdt = dgauss.table(sigma, tau)
    assert np.array_equal(table, cdt)
    for it in (1, 2):
        ids = srv.online_ids[it]
        n = len(ids)
        assert n == srv.online_counts[it] == N                       # the deterministic latency model loses no VECTOR
        ys = [l2.clip_forward(np.asarray(clients[i].input_vector, np.float32), norm, keys[it], h)[0] for i in ids]
        assert all(len(drew[(i, it)][0]) == 32 and len(drew[(i, it)][1]) == 32 for i in ids)
        Q = sum(G.quantised(y, f, c, cdt, drew[(i, it)][1], drew[(i, it)][0])[0] for i, y in zip(ids, ys))
        enc = sum(G.encode_any(y, f, c, P, cdt, drew[(i, it)][1], drew[(i, it)][0])[0].astype(np.uint64) for i, y in zip(ids, ys))
        S = (enc & 0xFFFFFFFF).astype(np.uint32)
        assert np.array_equal(srv.results[it], S)
        assert int(np.abs(Q).max()) < H                              # the premise: no sum wraps
        want, qh = MC.decode_mod(S, l_rot, f, P, n, Bn)
        assert np.array_equal(qh, Q)
        back = R.inverse(want, keys[it], h, L)
        assert srv.means[it].dtype == np.float32 and srv.means[it].tobytes() == back.tobytes()
        assert srv.near_wrap[it] == MC.stats(Q, H // 2)
    out = capsys.readouterr().out
    assert out.count("decoded modulo the field: H = 32768, guard = 16384, ") == 2
    assert out.count("discrete Gaussian noise sigma = 3.2, tail = 32: standard deviation of the difference") == 2
