"""The agents' distributed-DP option on the GPU: n = 32 clients, 1001 parameters in 501 words, two iterations with
--float_inputs 4,1,sr,pack2 --dp_noise 30, with and without three clients offline.  The claims of
tests/test_dp_protocol_cpu.py with the real engine: final_mean (VectorStore.unmask_unpack_f32 with noise_bits) is the
restatement's decode of the sum of the online clients' noised encodings, from the dither and noise seeds the
clients drew, bit for bit."""
import numpy as np
import pytest

import codec_cases as K
import dp_cases as D

pytestmark = pytest.mark.gpu

L = 1001


@pytest.mark.parametrize("offline", ["", "3,17,30"])
def test_noised_float_inputs_through_the_agents(monkeypatch, capsys, offline):
    from flamingo_amd.abides.config_flamingo import run
    from flamingo_amd.abides.flamingo import protocol
    from flamingo_amd.abides.flamingo.client_agent import SA_ClientAgent
    f, c, P, b = 4, 1.0, 2, 30
    drew = {}                                   # (client, iteration) -> (dither seed, noise seed): a client keeps its last
    vectors = SA_ClientAgent.sendVectors

    def send_vectors(self, *a, **kw):
        out = vectors(self, *a, **kw)
        drew[(self.id, self.current_iteration)] = (self.dither_seed, self.noise_seed)
        return out

    monkeypatch.setattr(SA_ClientAgent, "sendVectors", send_vectors)
    try:
        res = run(["-c", "flamingo", "-n", "32", "-i", "2", "-s", "11", "-k", "--committee_size", "9", "--vector_len", str(L),
                   "--float_inputs", "4,1,sr,pack2", "--dp_noise", "30"] + (["--offline", offline] if offline else []))
        assert protocol.codec_noise_bits() == b and protocol.codec_pack() == P and protocol.ring_len() == 501
    finally:
        protocol.configure(codec=False)
    srv, clients = res["server"], res["clients"]
    assert sorted(srv.means) == [1, 2]
    assert not offline or len(srv.recon_symbol) > 0              # dropout pairs were cancelled (a late VECTOR drops too)
    for it in (1, 2):
        ids = srv.online_ids[it]
        n = len(ids)
        assert 0 < n == srv.online_counts[it] <= (29 if offline else 32)
        mean, total = srv.means[it], srv.results[it]
        assert mean.dtype == np.float32 and mean.shape == (L,) and total.dtype == np.uint32 and total.shape == (501,)
        xs = [np.asarray(clients[i].input_vector, np.float32) for i in ids]
        assert all(clients[i].clipped == 0 and len(drew[(i, it)][1]) == 32 for i in ids)
        enc = sum(D.encode_packed_noised(x, f, c, P, drew[(i, it)][0], drew[(i, it)][1], b)[0].astype(np.uint64)
                  for i, x in zip(ids, xs))
        assert int(enc.max()) < 2 ** 32 and np.array_equal(total, enc.astype(np.uint32))
        assert mean.tobytes() == D.decode_packed_noised(enc.astype(np.uint32), L, f, c, P, b, n).tobytes()
        # the noise is the sum of the shares: with it taken out, the mean of the floats to within the rounding's step
        z = sum(D.noise(drew[(i, it)][1], L, b) for i in ids)
        plain = sum(K.encode(x, f, c, drew[(i, it)][0])[0].view(np.int32).astype(np.int64) for i, x in zip(ids, xs))
        assert mean.tobytes() == ((plain + z).astype(np.float64) / (np.float64(n) * 2.0 ** f)).astype(np.float32).tobytes()
        # 1001 samples: the estimate's relative standard deviation is 1 / sqrt(2 L) = 2.2 %, so 15 % is 6.7 sigma
        assert z.any() and abs(float(np.std(z / (n * 2.0 ** f))) / D.expected_std(f, b, n) - 1.0) < 0.15
    assert all(cl.noise_seed == drew[(cl.id, 2)][1] for cl in clients)
    out = capsys.readouterr().out
    assert out.count("standard deviation of the difference") == 2 and "noise of 30 coins" in out
