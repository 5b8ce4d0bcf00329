"""The agents' packed float inputs (--float_inputs F,CLIP[,sr],pack2|pack4; protocol.configure(codec=(f, c, mode,
pack))) on CPU: the engine stand-in of tests/test_codec_protocol_cpu.py with the numpy packed codec of
tests/pack_cases.py added.  vector_len stays the parameter count; the VECTOR bodies, the store and the sums are
ceil(vector_len / pack) words; final_mean has vector_len floats and is the restatement's decode of the summed
packed words, bit for bit.

Headroom, n 2 ceil(c 2^f) <= 2^(32/P) - 1 with the server's n = the number of clients:
  7,1,pack2:    32 x 2 x 128 = 8192 <= 65535: 32 clients fit;
  3,1,sr,pack4: 2B = 16, 255 // 16 = 15: 15 clients fit (15 x 16 = 240), 32 do not (512 > 255) -- the run of
                32 is the refusal case.  The simulation takes a power of two, so the pack4 runs take -n 8 with a
                committee of 5 (8 x 16 = 128); --offline 3,9,20 then names one client, so 3,5 runs as well.

Which VECTORs arrive late depends on the latency draws, and those on what earlier runs in the process left cached,
so the run against the unpacked codec uses --latency deterministic on both sides: nobody is late, U is the same."""
import numpy as np
import pytest

import codec_cases as K
import pack_cases as C
from test_codec_protocol_cpu import CodecEngine, CodecStore, _run

L = 1001


def argv(n):
    return ["-c", "flamingo", "-n", str(n), "-i", "2", "-s", "5", "-k", "--vector_len", str(L),
            "--committee_size", "9" if n >= 9 else "5", "--root_seed_hex", "11" * 32, "--round_time", "30"]


class PackStore(CodecStore):
    def unmask_unpack_f32(self, seeds, signs, L_params, frac_bits, clip, pack, count=1):
        if self.L != -(-L_params // pack):
            raise RuntimeError("flm_store_unmask_unpack_f32: wrong store length (code -1)")
        return C.decode_packed(self.unmask(seeds, signs), L_params, frac_bits, clip, pack, count)


class PackEngine(CodecEngine):
    def vector_store(self, L, capacity):
        return PackStore(L)

    def codec_check(self, frac_bits, clip, n_clients=1, pack=1):
        if pack == 1:
            return super().codec_check(frac_bits, clip, n_clients)
        if pack not in (2, 4):
            raise RuntimeError("flm_codec_check_packed: bad argument (code -1)")
        super().codec_check(frac_bits, clip, n_clients)
        if not C.headroom_ok(frac_bits, clip, pack, n_clients):
            raise RuntimeError("flm_codec_check_packed: a field can carry (code -4)")

    def client_encode_pack_mask(self, seg, seeds, signs, L, x, frac_bits, clip, pack, dither=None, return_clipped=False):
        self.codec_check(frac_bits, clip, 1, pack)
        rows, cl = [], []
        for i in range(len(seg) - 1):
            r, n = C.masked_packed(x[i], frac_bits, clip, pack, seeds[seg[i]:seg[i + 1]], signs[seg[i]:seg[i + 1]],
                                   dither[i] if dither is not None else None)
            rows.append(r)
            cl.append(n)
        out = np.stack(rows)
        return (out, np.array(cl, np.uint32)) if return_clipped else out

    def decode_unpack(self, total, L, frac_bits, clip, pack, count=1):
        return C.decode_packed(total, L, frac_bits, clip, pack, count)


@pytest.fixture
def pack_engine(monkeypatch):
    from flamingo_amd.abides.flamingo import protocol
    from flamingo_amd.abides.flamingo.client_agent import SA_ClientAgent
    monkeypatch.setattr(protocol, "_engine", PackEngine())
    sent = []
    send = SA_ClientAgent.sendMessage

    def record(self, recipient, msg, *a, **kw):
        if isinstance(msg.body, dict) and msg.body.get("msg") == "VECTOR":
            sent.append(dict(msg.body))
        return send(self, recipient, msg, *a, **kw)

    monkeypatch.setattr(SA_ClientAgent, "sendMessage", record)
    yield sent
    protocol.configure(committee=60, codec=False)


@pytest.mark.parametrize("n,spec,offline", [(32, "7,1,pack2", ""), (32, "7,1,pack2", "3,9,20"),
                                            (8, "3,1,sr,pack4", ""), (8, "3,1,sr,pack4", "3,9,20"),
                                            (8, "3,1,sr,pack4", "3,5")])
def test_final_mean_is_the_decode_of_the_summed_packed_words(pack_engine, capsys, n, spec, offline):
    from flamingo_amd.abides.flamingo import protocol
    parts = spec.split(",")
    f, c, P = int(parts[0]), float(parts[1]), int(parts[-1][4:])
    mode = "stochastic" if "sr" in parts else "nearest"
    Lw = -(-L // P)
    extra = ["--offline", offline] if offline else []
    res = _run(argv(n) + ["--float_inputs", spec] + extra)
    assert protocol.codec() == (f, c, mode) and protocol.codec_pack() == P and protocol.ring_len() == Lw
    assert protocol.vector_len == L
    srv, clients = res["server"], res["clients"]
    assert pack_engine and all(np.asarray(b["vector"]).shape == (Lw,) for b in pack_engine)      # the wire: Lw words
    assert sorted(srv.means) == [1, 2]
    dropped = len([i for i in offline.split(",") if i and int(i) < n])
    for it in (1, 2):
        ids = srv.online_ids[it]
        assert len(ids) == srv.online_counts[it] <= n - dropped
        assert C.headroom_ok(f, c, P, len(ids))
        mean, total = srv.means[it], srv.results[it]
        assert mean.dtype == np.float32 and mean.shape == (L,) and total.shape == (Lw,)
        assert mean.tobytes() == C.decode_packed(total, L, f, c, P, len(ids)).tobytes()
        xs = [np.asarray(clients[i].input_vector, np.float32) for i in ids]
        assert all(x.shape == (L,) and clients[i].clipped == 0 for i, x in zip(ids, xs))
        if mode == "nearest" or it == 2:        # a client keeps its last dither seed only
            enc = sum(C.encode_packed(x, f, c, P, clients[i].dither_seed)[0].astype(np.uint64) for i, x in zip(ids, xs))
            assert int(enc.max()) < 2 ** 32 and np.array_equal(total, enc.astype(np.uint32))
            assert mean.tobytes() == C.decode_packed(enc.astype(np.uint32), L, f, c, P, len(ids)).tobytes()
            # ... and the unpacked codec's decode of the unpacked sum of the same encodings
            plain = sum(K.encode(x, f, c, clients[i].dither_seed)[0].astype(np.uint64) for i, x in zip(ids, xs))
            assert mean.tobytes() == K.decode((plain & 0xFFFFFFFF).astype(np.uint32), f, len(ids)).tobytes()
        exact = np.mean([x.astype(np.float64) for x in xs], axis=0)
        err = np.abs(mean.astype(np.float64) - exact)
        # nearest, nothing clipped: at most half a step per element, so per mean, then one float32 rounding;
        # stochastic moves each element by less than one step
        bound = (2.0 ** -(f + 1) if mode == "nearest" else 2.0 ** -f) + 2.0 ** -24 * np.abs(exact)
        assert np.all(err <= bound), float(np.max(err - bound))
    assert (clients[0].dither_seed is not None) == (mode == "stochastic")
    out = capsys.readouterr().out
    assert out.count("largest |final_mean - mean of the clients' floats|") == 2 and f"{P} per word" in out


@pytest.mark.parametrize("offline", ["", "3,9,20"])
def test_nearest_mean_is_the_unpacked_runs_mean(pack_engine, offline):
    """The same inputs through the packed and the unpacked codec: the same means, byte for byte."""
    from flamingo_amd.abides.flamingo import protocol
    extra = ["--latency", "deterministic"] + (["--offline", offline] if offline else [])
    packed = _run(argv(32) + ["--float_inputs", "7,1,pack2"] + extra)["server"]
    assert protocol.codec_pack() == 2 and protocol.ring_len() == 501
    plain = _run(argv(32) + ["--float_inputs", "7,1"] + extra)["server"]
    assert protocol.codec_pack() == 1 and protocol.ring_len() == L
    for it in (1, 2):
        assert plain.online_ids[it] == packed.online_ids[it] and len(plain.online_ids[it]) == (29 if offline else 32)
        assert plain.results[it].shape == (L,) and packed.results[it].shape == (501,)
        assert plain.means[it].shape == (L,) and plain.means[it].tobytes() == packed.means[it].tobytes()


def test_server_refuses_a_run_without_packed_headroom(pack_engine):
    with pytest.raises(RuntimeError, match="code -4"):
        _run(argv(32) + ["--float_inputs", "3,1,sr,pack4"])       # 32 x 16 = 512 > 255
    with pytest.raises(RuntimeError, match="code -4"):
        _run(argv(32) + ["--float_inputs", "11,1,pack2"])         # 32 x 4096 = 131072 > 65535
    assert not pack_engine                                        # refused at set-up: nothing was sent
    for bad in ("7,1,pack3", "7,1,pack2,sr", "pack2", "7,pack2"):
        with pytest.raises(ValueError):
            _run(argv(32) + ["--float_inputs", bad])


def test_configure_takes_the_three_tuple_as_before():
    from flamingo_amd.abides.flamingo import protocol
    try:
        protocol.configure(L=L, codec=(7, 1.0, "nearest"))
        assert protocol.codec() == (7, 1.0, "nearest") and protocol.codec_pack() == 1 and protocol.ring_len() == L
        protocol.configure(codec=(7, 1.0, "stochastic", 4))
        assert protocol.codec() == (7, 1.0, "stochastic") and protocol.codec_pack() == 4 and protocol.ring_len() == 251
        protocol.configure(codec=(7, 1.0, "nearest", 1))
        assert protocol.codec_pack() == 1
        with pytest.raises(ValueError):
            protocol.configure(codec=(7, 1.0, "nearest", 3))
        protocol.configure(codec=False)
        assert protocol.codec() is None and protocol.codec_pack() == 1 and protocol.ring_len() == L
    finally:
        from flamingo_amd import params
        protocol.configure(L=params.vector_len, committee=60, codec=False)
