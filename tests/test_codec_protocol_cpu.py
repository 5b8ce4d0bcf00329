"""The agents' float-input option (protocol.configure(codec=...), --float_inputs) on CPU: the engine stand-in of
tests/test_abides_protocol_cpu.py with the numpy codec of tests/codec_cases.py added.  Two iterations, with and
without dropouts, nearest and stochastic: final_mean is the restatement's decode of the sum of the online clients'
encoded updates, bit for bit, and close to the mean of their floats; with the option off the VECTOR messages are
the ones the agents sent before the option existed."""
import hashlib

import numpy as np
import pytest

import codec_cases as K
from test_abides_protocol_cpu import OracleEngine, OracleStore

ARGV = ["-c", "flamingo", "-n", "32", "-i", "2", "-s", "5", "-k", "--vector_len", "1000",
        "--committee_size", "9", "--root_seed_hex", "11" * 32, "--round_time", "30"]
# SHA-256 over the VECTOR messages (sender, iteration, vector bytes, enc_mi_shares, enc_pairwise, in sending order)
# of ARGV + --offline 3,9,20, recorded from the agents as they were before the option was added
VECTOR_DIGEST_BEFORE = "2b7bde4d65d7da5b65edb866185386704b99c864803dd3935ef177cd021d1b9b"


class CodecStore(OracleStore):
    def unmask_f32(self, seeds, signs, frac_bits, count=1):
        return K.decode(self.unmask(seeds, signs), frac_bits, count)


class CodecEngine(OracleEngine):
    def vector_store(self, L, capacity):
        return CodecStore(L)

    def codec_check(self, frac_bits, clip, n_clients=1):
        if not (0 <= frac_bits <= 30 and 0 < clip < float("inf") and n_clients >= 1):
            raise RuntimeError("flm_codec_check: bad argument (code -1)")
        if not K.headroom_ok(frac_bits, clip, n_clients):
            raise RuntimeError("flm_codec_check: the sum can wrap (code -4)")

    def client_encode_mask(self, seg, seeds, signs, L, x, frac_bits, clip, dither=None, return_clipped=False):
        self.codec_check(frac_bits, clip, 1)
        rows, cl = [], []
        for i in range(len(seg) - 1):
            r, n = K.masked(x[i], frac_bits, clip, seeds[seg[i]:seg[i + 1]], signs[seg[i]:seg[i + 1]],
                            dither[i] if dither is not None else None)
            rows.append(r)
            cl.append(n)
        out = np.stack(rows)
        return (out, np.array(cl, np.uint32)) if return_clipped else out

    def decode_sum(self, total, frac_bits, count=1):
        return K.decode(total, frac_bits, count)


@pytest.fixture
def codec_engine(monkeypatch):
    from flamingo_amd.abides.flamingo import protocol
    from flamingo_amd.abides.flamingo.client_agent import SA_ClientAgent
    monkeypatch.setattr(protocol, "_engine", CodecEngine())
    sent = []
    send = SA_ClientAgent.sendMessage

    def record(self, recipient, msg, *a, **kw):
        if isinstance(msg.body, dict) and msg.body.get("msg") == "VECTOR":
            sent.append(dict(msg.body))
        return send(self, recipient, msg, *a, **kw)

    monkeypatch.setattr(SA_ClientAgent, "sendMessage", record)
    yield sent
    protocol.configure(committee=60, codec=False)


def _digest(sent):
    h = hashlib.sha256()
    for b in sent:
        h.update(repr((b["sender"], b["iteration"])).encode())
        h.update(np.asarray(b["vector"], np.uint32).tobytes())
        h.update(repr(b["enc_mi_shares"]).encode())
        h.update(repr(b["enc_pairwise"]).encode())
    return h.hexdigest()


def _run(argv):
    from flamingo_amd.abides.config_flamingo import run
    return run(argv)


@pytest.mark.parametrize("mode,offline", [("nearest", ""), ("nearest", "3,9,20"), ("stochastic", "3,9,20")])
def test_final_mean_is_the_decoded_sum_of_the_encoded_updates(codec_engine, capsys, mode, offline):
    f, c = 16, 4.0
    argv = ARGV + ["--float_inputs", f"{f},{c:g}" + (",sr" if mode == "stochastic" else "")]
    if offline:
        argv += ["--offline", offline]
    res = _run(argv)
    srv, clients = res["server"], res["clients"]
    assert sorted(srv.means) == [1, 2] and sorted(srv.results) == [1, 2]
    for it in (1, 2):
        ids = srv.online_ids[it]
        assert len(ids) == srv.online_counts[it] <= (29 if offline else 32)      # a late VECTOR drops its client too
        mean = srv.means[it]
        assert mean.dtype == np.float32 and mean.shape == (1000,)
        assert mean.tobytes() == K.decode(srv.results[it], f, len(ids)).tobytes()
        xs = [np.asarray(clients[i].input_vector, np.float32) for i in ids]
        assert all(x.dtype == np.float32 and clients[i].clipped == 0 for i, x in zip(ids, xs))
        if mode == "nearest" or it == 2:        # a client keeps its last dither seed only
            enc = sum(K.encode(x, f, c, clients[i].dither_seed)[0].astype(np.uint64) for i, x in zip(ids, xs))
            assert np.array_equal(srv.results[it], enc.astype(np.uint32))
            assert mean.tobytes() == K.decode(enc.astype(np.uint32), f, len(ids)).tobytes()
        exact = np.mean([x.astype(np.float64) for x in xs], axis=0)
        err = np.abs(mean.astype(np.float64) - exact)
        # nearest, nothing clipped: at most half a step per element, so per mean, then one float32 rounding;
        # stochastic moves each element by less than one step
        bound = (2.0 ** -(f + 1) if mode == "nearest" else 2.0 ** -f) + 2.0 ** -24 * np.abs(exact)
        assert np.all(err <= bound), float(np.max(err - bound))
    assert (clients[0].dither_seed is not None) == (mode == "stochastic")
    out = capsys.readouterr().out
    assert out.count("largest |final_mean - mean of the clients' floats|") == 2


def test_option_off_sends_what_was_sent_before(codec_engine):
    _run(ARGV + ["--offline", "3,9,20"])
    off = list(codec_engine)
    assert len(off) == 2 * 29 and _digest(off) == VECTOR_DIGEST_BEFORE
    # nearest adds no draw: every field but the vector is the same; stochastic draws its dither seed last, so the
    # first iteration's other fields are the same too
    for spec, its in (("16,4", (1, 2)), ("16,4,sr", (1,))):
        del codec_engine[:]
        _run(ARGV + ["--offline", "3,9,20", "--float_inputs", spec])
        on = list(codec_engine)
        assert [(b["sender"], b["iteration"]) for b in on] == [(b["sender"], b["iteration"]) for b in off]
        for a, b in zip(off, on):
            if a["iteration"] in its:
                assert a["enc_mi_shares"] == b["enc_mi_shares"] and a["enc_pairwise"] == b["enc_pairwise"]
            assert not np.array_equal(a["vector"], b["vector"])


def test_server_refuses_a_run_without_headroom(codec_engine):
    with pytest.raises(RuntimeError, match="code -4"):
        _run(ARGV + ["--float_inputs", "30,1"])           # 32 clients of magnitude 2^30
    with pytest.raises(ValueError):
        _run(ARGV + ["--float_inputs", "16"])
