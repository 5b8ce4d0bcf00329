"""The agents' discrete Gaussian option on the GPU: n = 128 clients, 1001 parameters, two iterations with
--float_inputs 4,1,sr,pack2 --rotate 5 --l2_clip 2.28125 --round_bound 1 --dp_gauss 3.2.  Replayed on the CPU from the
dither and noise seeds the clients recorded -- tests/l2_cases.py in front of tests/rotate_cases.py, then
tests/dgauss_cases.py: final_mean is the inverse rotation of the restatement's decode of the sum of the online clients'
noised rows, bit for bit.  Without --dp_gauss the same run draws no noise seed, calls no table-mode encode and is the
pipeline without noise that tests/test_round_abides_gpu.py pins, replayed here in the same process."""
import numpy as np
import pytest

import dgauss_cases as G
import l2_cases as l2
import pack_cases as PC
import rotate_cases as R

pytestmark = pytest.mark.gpu

N, L, F, C, P, H = 128, 1001, 4, 1.0, 2, 5
L_ROT = 1024
NORM = 2.28125
SIGMA, TAU = 3.2, 32


def _run(monkeypatch, extra):
    from flamingo_amd import MaskEngine
    from flamingo_amd.abides.config_flamingo import run
    from flamingo_amd.abides.flamingo import protocol
    from flamingo_amd.abides.flamingo.client_agent import SA_ClientAgent
    drew, calls = {}, []    # (client, iteration) -> (dither seed, noise seed)
    vectors, gauss = SA_ClientAgent.sendVectors, MaskEngine.client_encode_gauss_mask

    def encode_gauss(self, *a, **kw):
        calls.append(1)
        return gauss(self, *a, **kw)

    def send_vectors(self, *a, **kw):
        out = vectors(self, *a, **kw)
        drew[(self.id, self.current_iteration)] = (self.dither_seed, self.noise_seed)
        return out

    with monkeypatch.context() as m:
        m.setattr(SA_ClientAgent, "sendVectors", send_vectors)
        m.setattr(MaskEngine, "client_encode_gauss_mask", encode_gauss)
        try:
            res = run(["-c", "flamingo", "-n", str(N), "-i", "2", "-s", "11", "-k", "--committee_size", "9",
                       "--vector_len", str(L), "--float_inputs", "4,1,sr,pack2", "--rotate", str(H), "--l2_clip", str(NORM),
                       "--round_bound", "1"] + extra)
            state = (protocol.dp_gauss(), protocol.decode_noise_bits(), protocol.codec_noise_bits(), protocol.rotated_len(),
                     protocol.ring_len())
            table = protocol.dp_gauss_table()
            keys = {it: protocol.rotation_key(it) for it in (1, 2)}
        finally:
            protocol.configure(codec=False)
    return res["server"], res["clients"], drew, len(calls), state, table, keys


def test_dp_gauss_through_the_agents(monkeypatch, capsys):
    from flamingo_amd import dgauss
    srv, clients, drew, calls, state, table, keys = _run(monkeypatch, ["--dp_gauss", str(SIGMA)])
    assert state == ((SIGMA, TAU), 2 * TAU, 0, L_ROT, L_ROT // 2)
    cdt = dgauss.table(SIGMA, TAU)
    assert np.array_equal(table, cdt)
    var = float(dgauss.moments(cdt)[1])
    for it in (1, 2):
        ids = srv.online_ids[it]
        n = len(ids)
        assert 0 < n == srv.online_counts[it] <= N
        ys = [l2.clip_forward(np.asarray(clients[i].input_vector, np.float32), NORM, keys[it], H)[0] for i in ids]
        assert all(len(drew[(i, it)][0]) == 32 and len(drew[(i, it)][1]) == 32 for i in ids)
        enc = sum(G.encode_any(y, F, C, P, cdt, drew[(i, it)][1], drew[(i, it)][0])[0].astype(np.uint64) for i, y in zip(ids, ys))
        assert int(enc.max()) < 2 ** 32 and np.array_equal(srv.results[it], enc.astype(np.uint32))
        back = R.inverse(G.decode_any(enc.astype(np.uint32), L_ROT, F, C, P, TAU, n), keys[it], H, L)
        assert srv.means[it].dtype == np.float32 and srv.means[it].tobytes() == back.tobytes()
        # the noise in the sum is the sum of the shares; 1024 samples: the estimate's relative standard deviation is
        # 1 / sqrt(2 L) = 2.2 %, so 15 % is 6.8 sigma
        z = sum(G.noise(drew[(i, it)][1], L_ROT, cdt) for i in ids)
        assert z.any() and abs(float(np.std(z)) / np.sqrt(n * var) - 1.0) < 0.15
    assert sum(srv.online_counts[it] for it in (1, 2)) <= calls == len(drew) <= 2 * N   # one table-mode call per VECTOR
    assert all(cl.noise_seed == drew[(cl.id, 2)][1] for cl in clients if (cl.id, 2) in drew)
    out = capsys.readouterr().out
    assert out.count("discrete Gaussian noise sigma = 3.2, tail = 32: standard deviation of the difference") == 2
    assert out.count("expected sqrt(|U| Var) / (|U| 2^f) = ") == 2


def test_without_dp_gauss_the_run_is_unchanged(monkeypatch, capsys):
    srv, clients, drew, calls, state, table, keys = _run(monkeypatch, [])
    assert state == (None, 0, 0, L_ROT, L_ROT // 2) and table is None and calls == 0
    for it in (1, 2):
        ids = srv.online_ids[it]
        assert all(len(drew[(i, it)][0]) == 32 and drew[(i, it)][1] is None for i in ids)      # no noise seed drawn
        ys = [l2.clip_forward(np.asarray(clients[i].input_vector, np.float32), NORM, keys[it], H)[0] for i in ids]
        enc = sum(PC.encode_packed(y, F, C, P, drew[(i, it)][0])[0].astype(np.uint64) for i, y in zip(ids, ys))
        assert int(enc.max()) < 2 ** 32 and np.array_equal(srv.results[it], enc.astype(np.uint32))
        back = R.inverse(PC.decode_packed(enc.astype(np.uint32), L_ROT, F, C, P, len(ids)), keys[it], H, L)
        assert srv.means[it].tobytes() == back.tobytes()
    out = capsys.readouterr().out
    assert "discrete Gaussian" not in out and "noise of" not in out
