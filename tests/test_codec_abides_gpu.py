"""The agents' float-input option on the GPU: n = 128 clients, L = 4096, two iterations with --float_inputs 16,4
(and three clients offline).  The claims of tests/test_codec_protocol_cpu.py, with the real engine: final_mean
(VectorStore.unmask_f32) is the restatement's decode of the sum of the online clients' encoded updates, bit for
bit, and within half a step plus one float32 rounding of the mean of their floats."""
import numpy as np
import pytest

import codec_cases as K

pytestmark = pytest.mark.gpu


def test_float_inputs_through_the_agents():
    from flamingo_amd.abides.config_flamingo import run
    from flamingo_amd.abides.flamingo import protocol
    f, c = 16, 4.0
    try:
        res = run(["-c", "flamingo", "-n", "128", "-i", "2", "-s", "11", "-k", "--offline", "3,77,100",
                   "--vector_len", "4096", "--float_inputs", "16,4"])
    finally:
        protocol.configure(codec=False)
    srv, clients = res["server"], res["clients"]
    assert sorted(srv.means) == [1, 2]
    assert len(srv.recon_symbol) > 0          # dropout pairs were cancelled
    for it in (1, 2):
        ids = srv.online_ids[it]
        assert 0 < len(ids) == srv.online_counts[it] <= 125
        mean, total = srv.means[it], srv.results[it]
        assert mean.dtype == np.float32 and mean.shape == (4096,) and total.dtype == np.uint32
        xs = [np.asarray(clients[i].input_vector, np.float32) for i in ids]
        assert all(clients[i].clipped == 0 for i in ids)
        enc = sum(K.encode(x, f, c)[0].astype(np.uint64) for x in xs).astype(np.uint32)
        assert np.array_equal(total, enc)
        assert mean.tobytes() == K.decode(enc, f, len(ids)).tobytes()
        exact = np.mean([x.astype(np.float64) for x in xs], axis=0)
        err = np.abs(mean.astype(np.float64) - exact)
        assert np.all(err <= 2.0 ** -(f + 1) + 2.0 ** -24 * np.abs(exact)), float(err.max())
