"""The agents' L2 clip on the GPU: n = 128 clients, 4001 parameters, two iterations with
--float_inputs 7,1,sr,pack2 --rotate 5 --l2_clip 2.28125 and three clients offline.  The synthetic updates have norms
2.225-2.321 (median 2.286), so about half the cohort is scaled.  With the real engine final_mean is the restated
pipeline bit for bit -- tests/l2_cases.py in front of tests/rotate_cases.py around tests/pack_cases.py, from the dither
seeds the clients drew and the iteration's rotation key -- and every client's l2_norm and l2_factor are the
restatement's.  Without --l2_clip the same run is what tests/test_rotate_abides_gpu.py pins; without --rotate the clip
is the standalone pass in front of the packed codec."""
import numpy as np
import pytest

import l2_cases as l2
import pack_cases as PC
import rotate_cases as R

pytestmark = pytest.mark.gpu

L, F, C, P, H = 4001, 7, 1.0, 2, 5
NORM = 2.28125


def _run(monkeypatch, extra):
    from flamingo_amd.abides.config_flamingo import run
    from flamingo_amd.abides.flamingo import protocol
    from flamingo_amd.abides.flamingo.client_agent import SA_ClientAgent
    drew = {}               # (client, iteration) -> (dither seed, clipped, non-finite, l2_factor, l2_norm)
    vectors = SA_ClientAgent.sendVectors

    def send_vectors(self, *a, **kw):
        out = vectors(self, *a, **kw)
        drew[(self.id, self.current_iteration)] = (self.dither_seed, self.clipped, self.nonfinite, self.l2_factor, self.l2_norm)
        return out

    monkeypatch.setattr(SA_ClientAgent, "sendVectors", send_vectors)
    try:
        res = run(["-c", "flamingo", "-n", "128", "-i", "2", "-s", "11", "-k", "--offline", "3,77,100",
                   "--vector_len", str(L), "--float_inputs", "7,1,sr,pack2"] + extra)
        shape = (protocol.rotate_bits(), protocol.rotated_len(), protocol.ring_len(), protocol.l2_clip())
        keys = {it: protocol.rotation_key(it) for it in (1, 2)}
    finally:
        protocol.configure(codec=False)
    return res["server"], res["clients"], drew, shape, keys


def test_l2_clipped_rotated_float_inputs_through_the_agents(monkeypatch, capsys):
    srv, clients, drew, shape, keys = _run(monkeypatch, ["--rotate", str(H), "--l2_clip", str(NORM)])
    assert shape == (H, 4032, 2016, NORM) and srv.ring_len == 2016
    assert sorted(srv.means) == [1, 2]
    counts = []
    for it in (1, 2):
        ids = srv.online_ids[it]
        n = len(ids)
        assert 0 < n == srv.online_counts[it] <= 125
        mean, total = srv.means[it], srv.results[it]
        assert mean.dtype == np.float32 and mean.shape == (L,) and total.shape == (2016,)
        xs = [np.asarray(clients[i].input_vector, np.float32) for i in ids]
        want = [l2.clip_forward(x, NORM, keys[it], H) for x in xs]
        for i, (y, bad, s, S) in zip(ids, want):                                  # l2_factor and l2_norm per client
            assert drew[(i, it)][1:] == (0, 0, float(s), float(np.sqrt(S))), i    # clipped == nonfinite == 0
        scaled = sum(drew[(i, it)][3] < 1.0 for i in ids)
        assert scaled >= 10 and sum(drew[(i, it)][3] == 1.0 for i in ids) >= 10 and scaled + 10 <= n
        counts.append((scaled, n))
        enc = sum(PC.encode_packed(y, F, C, P, drew[(i, it)][0])[0].astype(np.uint64) for i, (y, _, _, _) in zip(ids, want))
        assert int(enc.max()) < 2 ** 32 and np.array_equal(total, enc.astype(np.uint32))
        back = R.inverse(PC.decode_packed(enc.astype(np.uint32), 4032, F, C, P, n), keys[it], H, L)
        assert mean.tobytes() == back.tobytes()
        # the mean of the clipped updates, within the rotated codec's sqrt(32) steps and the transforms' rounding
        exact = np.mean([l2.clip(x, NORM)[0].astype(np.float64) for x in xs], axis=0)
        assert np.max(np.abs(mean.astype(np.float64) - exact)) <= np.sqrt(32.0) * 2.0 ** -F + 1e-5
        norms = [float(np.linalg.norm(l2.clip(x, NORM)[0].astype(np.float64))) for x in xs]
        assert max(norms) <= NORM * l2.BOUND
    out = capsys.readouterr().out
    for k, n in counts:
        assert f"0 elements clipped, 0 non-finite, {k} of {n} clients scaled to norm 2.28125" in out
    assert out.count("clients scaled to norm") == 2


def test_without_l2_clip_the_rotated_run_is_unchanged(monkeypatch, capsys):
    srv, clients, drew, shape, keys = _run(monkeypatch, ["--rotate", str(H)])
    assert shape == (H, 4032, 2016, None) and srv.ring_len == 2016
    for it in (1, 2):
        ids = srv.online_ids[it]
        n = len(ids)
        mean, total = srv.means[it], srv.results[it]
        assert all(drew[(i, it)][1:] == (0, 0, None, None) for i in ids)
        xs = [np.asarray(clients[i].input_vector, np.float32) for i in ids]
        ys = [R.forward(x, keys[it], H)[0] for x in xs]
        enc = sum(PC.encode_packed(y, F, C, P, drew[(i, it)][0])[0].astype(np.uint64) for i, y in zip(ids, ys))
        assert np.array_equal(total, enc.astype(np.uint32))
        want = R.inverse(PC.decode_packed(enc.astype(np.uint32), 4032, F, C, P, n), keys[it], H, L)
        assert mean.tobytes() == want.tobytes()
    out = capsys.readouterr().out
    assert out.count("rotated in blocks of 2^5") == 2 and out.count("0 elements clipped, 0 non-finite\n") == 2
    assert "scaled to norm" not in out


def test_l2_clip_without_the_rotation(monkeypatch, capsys):
    # the unrotated synthetic updates are normal draws of deviation 1 / 8: norms about 7.9, on both sides of it
    srv, clients, drew, shape, _ = _run(monkeypatch, ["--l2_clip", "7.9"])
    assert shape == (0, L, 2001, float(np.float32(7.9))) and srv.ring_len == 2001
    for it in (1, 2):
        ids = srv.online_ids[it]
        n = len(ids)
        mean, total = srv.means[it], srv.results[it]
        xs = [np.asarray(clients[i].input_vector, np.float32) for i in ids]
        want = [l2.clip(x, 7.9) for x in xs]
        for i, (y, s, S) in zip(ids, want):
            assert drew[(i, it)][2:] == (0, float(s), float(np.sqrt(S))), i
        assert sum(s < 1.0 for _, s, _ in want) >= 10 and sum(s == 1.0 for _, s, _ in want) >= 10
        packed = [PC.encode_packed(y, F, C, P, drew[(i, it)][0]) for i, (y, _, _) in zip(ids, want)]
        assert [int(cl.sum()) for _, cl in packed] == [drew[(i, it)][1] for i in ids]
        enc = sum(w.astype(np.uint64) for w, _ in packed)
        assert np.array_equal(total, enc.astype(np.uint32))
        assert mean.tobytes() == PC.decode_packed(enc.astype(np.uint32), L, F, C, P, n).tobytes()
    out = capsys.readouterr().out
    assert out.count("clients scaled to norm 7.9") == 2 and "rotated" not in out
