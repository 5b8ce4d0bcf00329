"""The agents' rotation option on the GPU: n = 128 clients, 4001 parameters, two iterations with
--float_inputs 7,1,sr,pack2 --rotate 5 and three clients offline.  With the real engine: the VECTOR bodies and the sums
are ring_len = ceil(round_up(4001, 32) / 2) = 2016 words, no online client clips or holds a non-finite value, and
final_mean (the store's packed decode, rotated back by MaskEngine.rotate) has 4001 entries and is the restated pipeline
bit for bit: tests/rotate_cases.py around tests/pack_cases.py, from the dither seeds the clients drew and the
iteration's rotation key.  Without --rotate the same run is the packed codec's pipeline alone, 2001 words a body."""
import numpy as np
import pytest

import pack_cases as PC
import rotate_cases as R

pytestmark = pytest.mark.gpu

L, F, C, P, H = 4001, 7, 1.0, 2, 5


def _run(monkeypatch, extra):
    from flamingo_amd.abides.config_flamingo import run
    from flamingo_amd.abides.flamingo import protocol
    from flamingo_amd.abides.flamingo.client_agent import SA_ClientAgent
    drew = {}                                   # (client, iteration) -> (dither seed, clipped, non-finite): a client keeps its last
    vectors = SA_ClientAgent.sendVectors

    def send_vectors(self, *a, **kw):
        out = vectors(self, *a, **kw)
        drew[(self.id, self.current_iteration)] = (self.dither_seed, self.clipped, self.nonfinite)
        return out

    monkeypatch.setattr(SA_ClientAgent, "sendVectors", send_vectors)
    try:
        res = run(["-c", "flamingo", "-n", "128", "-i", "2", "-s", "11", "-k", "--offline", "3,77,100",
                   "--vector_len", str(L), "--float_inputs", "7,1,sr,pack2"] + extra)
        shape = (protocol.rotate_bits(), protocol.rotated_len(), protocol.ring_len())
        keys = {it: protocol.rotation_key(it) for it in (1, 2)}
    finally:
        protocol.configure(codec=False)
    return res["server"], res["clients"], drew, shape, keys


def test_rotated_float_inputs_through_the_agents(monkeypatch, capsys):
    srv, clients, drew, shape, keys = _run(monkeypatch, ["--rotate", str(H)])
    assert shape == (H, 4032, 2016) and srv.ring_len == 2016
    assert sorted(srv.means) == [1, 2] and len(srv.recon_symbol) > 0
    for it in (1, 2):
        ids = srv.online_ids[it]
        n = len(ids)
        assert 0 < n == srv.online_counts[it] <= 125
        mean, total = srv.means[it], srv.results[it]
        assert mean.dtype == np.float32 and mean.shape == (L,) and total.dtype == np.uint32 and total.shape == (2016,)
        assert all(drew[(i, it)][1] == 0 and drew[(i, it)][2] == 0 for i in ids)          # clipped == nonfinite == 0
        xs = [np.asarray(clients[i].input_vector, np.float32) for i in ids]
        assert all(x.shape == (L,) for x in xs)
        ys = [R.forward(x, keys[it], H)[0] for x in xs]
        enc = sum(PC.encode_packed(y, F, C, P, drew[(i, it)][0])[0].astype(np.uint64) for i, y in zip(ids, ys))
        assert int(enc.max()) < 2 ** 32 and np.array_equal(total, enc.astype(np.uint32))
        want = R.inverse(PC.decode_packed(enc.astype(np.uint32), 4032, F, C, P, n), keys[it], H, L)
        assert mean.tobytes() == want.tobytes()
        # stochastic rounding: every rotated coordinate of the mean within a step, so every original one within
        # sqrt(32) steps in the worst case, plus the two transforms' rounding
        exact = np.mean([x.astype(np.float64) for x in xs], axis=0)
        assert np.max(np.abs(mean.astype(np.float64) - exact)) <= np.sqrt(32.0) * 2.0 ** -F + 1e-5
    assert keys[1] != keys[2]
    out = capsys.readouterr().out
    assert out.count("rotated in blocks of 2^5") == 2 and out.count("0 elements clipped, 0 non-finite") == 2


def test_without_rotate_nothing_changed(monkeypatch, capsys):
    srv, clients, drew, shape, _ = _run(monkeypatch, [])
    assert shape == (0, L, 2001) and srv.ring_len == 2001
    for it in (1, 2):
        ids = srv.online_ids[it]
        n = len(ids)
        mean, total = srv.means[it], srv.results[it]
        assert mean.shape == (L,) and total.shape == (2001,)
        xs = [np.asarray(clients[i].input_vector, np.float32) for i in ids]
        enc = sum(PC.encode_packed(x, F, C, P, drew[(i, it)][0])[0].astype(np.uint64) for i, x in zip(ids, xs))
        assert np.array_equal(total, enc.astype(np.uint32))
        assert mean.tobytes() == PC.decode_packed(enc.astype(np.uint32), L, F, C, P, n).tobytes()
        assert all(drew[(i, it)][1:] == (0, 0) for i in ids)
    from flamingo_amd.synthetic import float_update
    assert all(np.array_equal(clients[i].input_vector, float_update(i, L, C)) for i in srv.online_ids[2])
    out = capsys.readouterr().out
    assert "rotated" not in out and "non-finite" not in out
