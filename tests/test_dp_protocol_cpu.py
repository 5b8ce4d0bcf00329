"""The agents' distributed-DP option (--dp_noise BITS; protocol.configure(dp_noise=b)) on CPU: the engine stand-in
of tests/test_pack_protocol_cpu.py with the numpy noise of tests/dp_cases.py added.  The option needs the float
inputs; the server refuses a run without noised headroom at set-up; with the noise off a run sends and draws what
it did before the option existed, through engines that know nothing of it; with it on the noise seed is each
client's last draw and final_mean is the restatement's decode of the sum of the clients' noised encodings.

Headroom with the server's n = the number of clients, B_n = ceil(c 2^f) + b / 2:
  4,1,sr,pack2 with b = 30: 32 x 2 x 31 = 1984 <= 65535;     16,4 with b = 64: 32 x 262176 <= 2^31 - 1;
  3,1,pack4 with 8 clients: 8 x 2 x (8 + b / 2) <= 255 holds up to b = 14 (8 x 2 x 15 = 240) and not at b = 16."""
import numpy as np
import pytest

import codec_cases as K
import dp_cases as D
from test_codec_protocol_cpu import _digest, _run
from test_pack_protocol_cpu import PackEngine, PackStore, argv

L = 1001
DET = ["--latency", "deterministic"]


class DpStore(PackStore):
    def unmask_unpack_f32(self, seeds, signs, L_params, frac_bits, clip, pack, count=1, noise_bits=0):
        if noise_bits == 0:
            return super().unmask_unpack_f32(seeds, signs, L_params, frac_bits, clip, pack, count)
        if self.L != -(-L_params // pack):
            raise RuntimeError("flm_store_unmask_unpack_noise_f32: wrong store length (code -1)")
        return D.decode_packed_noised(self.unmask(seeds, signs), L_params, frac_bits, clip, pack, noise_bits, count)


class DpEngine(PackEngine):
    def __init__(self):
        super().__init__()
        self.calls = []

    def vector_store(self, L, capacity):
        return DpStore(L)

    def codec_check(self, frac_bits, clip, n_clients=1, pack=1, noise_bits=0, L=0):
        self.calls.append(("codec_check", noise_bits))
        if noise_bits == 0:
            return super().codec_check(frac_bits, clip, n_clients, pack)
        if pack not in (1, 2, 4) or noise_bits < 0 or noise_bits > 1024 or noise_bits % 2:
            raise RuntimeError("flm_codec_check_noise: bad argument (code -1)")
        super().codec_check(frac_bits, clip, n_clients, pack)
        if not D.headroom_ok(frac_bits, clip, pack, noise_bits, n_clients) or not D.length_ok(noise_bits, L):
            raise RuntimeError("flm_codec_check_noise: no headroom (code -4)")

    def client_encode_noise_mask(self, seg, seeds, signs, L, x, frac_bits, clip, pack=1, dither=None, noise_bits=0,
                                 noise=None, return_clipped=False):
        self.calls.append(("client_encode_noise_mask", noise_bits))
        self.codec_check(frac_bits, clip, 1, pack, noise_bits, L)
        if noise_bits and noise is None:
            raise RuntimeError("flm_client_encode_noise_mask: noise is NULL (code -1)")
        rows, cl = [], []
        for i in range(len(seg) - 1):
            r, n = D.masked_noised(x[i], frac_bits, clip, pack, seeds[seg[i]:seg[i + 1]], signs[seg[i]:seg[i + 1]],
                                   dither[i] if dither is not None else None, noise[i] if noise_bits else None, noise_bits)
            rows.append(r)
            cl.append(n)
        out = np.stack(rows)
        return (out, np.array(cl, np.uint32)) if return_clipped else out

    def decode_unpack(self, total, L, frac_bits, clip, pack, count=1, noise_bits=0):
        return D.decode_packed_noised(total, L, frac_bits, clip, pack, noise_bits, count)


def _fixture(monkeypatch, engine):
    """The engine stand-in, the VECTOR bodies as sent, and per (client, iteration) what sendVectors drew and left."""
    from flamingo_amd.abides.flamingo import protocol
    from flamingo_amd.abides.flamingo.client_agent import SA_ClientAgent
    monkeypatch.setattr(protocol, "_engine", engine)
    sent, drew = [], {}
    send, vectors = SA_ClientAgent.sendMessage, SA_ClientAgent.sendVectors

    def record(self, recipient, msg, *a, **kw):
        if isinstance(msg.body, dict) and msg.body.get("msg") == "VECTOR":
            sent.append(dict(msg.body))
        return send(self, recipient, msg, *a, **kw)

    def send_vectors(self, *a, **kw):
        out = vectors(self, *a, **kw)
        drew[(self.id, self.current_iteration)] = (self.dither_seed, getattr(self, "noise_seed", None),
                                                   self.random_state.get_state())
        return out

    monkeypatch.setattr(SA_ClientAgent, "sendMessage", record)
    monkeypatch.setattr(SA_ClientAgent, "sendVectors", send_vectors)
    return sent, drew


@pytest.fixture
def dp(monkeypatch):
    from flamingo_amd.abides.flamingo import protocol
    engine = DpEngine()
    sent, drew = _fixture(monkeypatch, engine)
    yield engine, sent, drew
    protocol.configure(committee=60, codec=False)


@pytest.fixture
def plain(monkeypatch):
    """An engine that knows nothing of the noise: tests/test_pack_protocol_cpu.py's, its signatures as they are."""
    from flamingo_amd.abides.flamingo import protocol
    sent, drew = _fixture(monkeypatch, PackEngine())
    yield sent, drew
    protocol.configure(committee=60, codec=False)


def _same_state(a, b):
    return a[0] == b[0] and np.array_equal(a[1], b[1]) and a[2:] == b[2:]


# ------------------------------------------------------------------ the option
def test_option_parsing(dp):
    from flamingo_amd.abides.flamingo import protocol
    engine, sent, _ = dp
    with pytest.raises(ValueError, match="float"):
        _run(argv(32) + ["--dp_noise", "30"])                                  # needs --float_inputs
    for bad in ("31", "1026", "-2"):
        with pytest.raises(ValueError, match="even"):
            _run(argv(32) + ["--float_inputs", "4,1,pack2", "--dp_noise", bad])
    assert not sent
    try:
        protocol.configure(L=L, codec=(4, 1.0, "nearest", 2), dp_noise=30)
        assert protocol.codec_noise_bits() == 30 and protocol.codec_pack() == 2
        protocol.configure(dp_noise=0)
        assert protocol.codec_noise_bits() == 0 and protocol.codec() == (4, 1.0, "nearest")
        protocol.configure(dp_noise=2)
        protocol.configure(codec=False)                                        # the float inputs off: the noise with them
        assert protocol.codec_noise_bits() == 0
        with pytest.raises(ValueError):
            protocol.configure(dp_noise=2)
        assert protocol.codec_noise_bits() == 0
    finally:
        from flamingo_amd import params
        protocol.configure(L=params.vector_len, committee=60, codec=False)


def test_server_refuses_a_run_without_noised_headroom(dp):
    engine, sent, _ = dp
    with pytest.raises(RuntimeError, match="code -4"):
        _run(argv(8) + ["--float_inputs", "3,1,pack4", "--dp_noise", "16"])     # 8 x 2 x 16 = 256 > 255
    with pytest.raises(RuntimeError, match="code -4"):
        _run(argv(64) + ["--float_inputs", "7,1,pack2", "--dp_noise", "1024"])      # 64 x 2 x 640 > 65535
    assert not sent and ("codec_check", 16) in engine.calls                      # refused at set-up: nothing was sent
    _run(argv(8) + ["--float_inputs", "3,1,pack4", "--dp_noise", "14"])         # 8 x 2 x 15 = 240: runs
    assert sent


# ------------------------------------------------------------------ noise off
@pytest.mark.parametrize("spec", ["4,1,sr,pack2", "16,4,sr"])
def test_noise_off_sends_and_draws_what_was_sent_and_drawn(plain, spec):
    """--dp_noise 0 and the option absent, on the same seed, through an engine whose methods have the signatures they
    had before the option: the same VECTOR messages, the same dither seeds, the same generator states."""
    sent, drew = plain
    base = argv(32) + DET + ["--offline", "3,9,20", "--float_inputs", spec]
    _run(base)
    absent, absent_drew = list(sent), dict(drew)
    del sent[:]
    drew.clear()
    _run(base + ["--dp_noise", "0"])
    assert len(absent) == 2 * 29 == len(sent) and _digest(sent) == _digest(absent)
    assert sorted(drew) == sorted(absent_drew)
    for key, (dither, noise, state) in drew.items():
        assert dither == absent_drew[key][0] and (dither is None) == (key[0] in (3, 9, 20)) and noise is None
        assert _same_state(state, absent_drew[key][2])


# ------------------------------------------------------------------ noise on
@pytest.mark.parametrize("spec,b,offline", [("4,1,sr,pack2", 30, "3,9,20"), ("16,4", 64, ""), ("16,4,sr", 2, "3,9,20")])
def test_noise_on(dp, capsys, spec, b, offline):
    from flamingo_amd.abides.flamingo import protocol
    engine, sent, drew = dp
    parts = spec.split(",")
    f, c = int(parts[0]), float(parts[1])
    P = int(parts[-1][4:]) if parts[-1].startswith("pack") else 1
    base = argv(32) + DET + (["--offline", offline] if offline else []) + ["--float_inputs", spec]
    _run(base)                                                                   # the same seed without noise
    off_sent, off_drew = list(sent), dict(drew)
    assert not any(name == "client_encode_noise_mask" for name, _ in engine.calls)
    del sent[:], engine.calls[:]
    drew.clear()
    res = _run(base + ["--dp_noise", str(b)])
    assert protocol.codec_noise_bits() == b
    assert ("codec_check", b) in engine.calls and ("client_encode_noise_mask", b) in engine.calls
    srv, clients = res["server"], res["clients"]
    # the noise seed is each client's last draw: up to it the first iteration draws what the run without noise drew
    # (the other fields of its VECTOR messages are the same), the seed is the next 32 bytes of the generator as that
    # run left it, and nothing is drawn after it
    first = [b_ for b_ in sent if b_["iteration"] == 1]
    assert len(first) == len([b_ for b_ in off_sent if b_["iteration"] == 1]) > 0
    for a, b_ in zip([m for m in off_sent if m["iteration"] == 1], first):
        assert a["sender"] == b_["sender"] and a["enc_mi_shares"] == b_["enc_mi_shares"] and a["enc_pairwise"] == b_["enc_pairwise"]
        assert not np.array_equal(a["vector"], b_["vector"])
        dither, noise, state = drew[(b_["sender"], 1)]
        off_dither, off_noise, off_state = off_drew[(b_["sender"], 1)]
        assert dither == off_dither and off_noise is None and len(noise) == 32
        g = np.random.RandomState()
        g.set_state(off_state)
        assert noise == bytes(g.randint(0, 256, size=32, dtype=np.uint8))
        assert _same_state(g.get_state(), state)
    # final_mean from the clients' recorded inputs, dither seeds and noise seeds
    assert sorted(srv.means) == [1, 2]
    for it in (1, 2):
        ids = srv.online_ids[it]
        n = len(ids)
        assert n == srv.online_counts[it] == (29 if offline else 32) and D.headroom_ok(f, c, P, b, n)
        xs = [np.asarray(clients[i].input_vector, np.float32) for i in ids]
        enc = sum(D.encode_any(x, f, c, P, drew[(i, it)][0], drew[(i, it)][1], b)[0].astype(np.uint64) for i, x in zip(ids, xs))
        total = (enc & 0xFFFFFFFF).astype(np.uint32)
        assert np.array_equal(srv.results[it], total)
        mean = srv.means[it]
        assert mean.dtype == np.float32 and mean.shape == (L,)
        assert mean.tobytes() == D.decode_any(total, L, f, c, P, b, n).tobytes()
        # against the mean of the floats: the rounding's step and the summed noise, at most n b / 2 over n 2^f
        exact = np.mean([x.astype(np.float64) for x in xs], axis=0)
        z = sum(D.noise(drew[(i, it)][1], L, b) for i in ids)
        plain = sum(K.encode(x, f, c, drew[(i, it)][0])[0].view(np.int32).astype(np.int64) for i, x in zip(ids, xs))
        assert mean.tobytes() == ((plain + z).astype(np.float64) / (np.float64(n) * 2.0 ** f)).astype(np.float32).tobytes()
        err = np.abs(mean.astype(np.float64) - z / (n * 2.0 ** f) - exact)
        assert np.all(err <= 2.0 ** -f + 2.0 ** -22 * (np.abs(exact) + b)), float(err.max())
    assert all(cl.noise_seed == drew[(cl.id, 2)][1] for cl in clients if (cl.id, 2) in drew)
    out = capsys.readouterr().out
    assert out.count("standard deviation of the difference") == 2 and f"noise of {b} coins" in out
