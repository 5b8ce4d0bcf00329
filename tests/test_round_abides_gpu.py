"""The agents' conditional stochastic rounding on the GPU: n = 16 clients, 1001 parameters, two iterations with
--float_inputs 7,1,sr,pack2 --rotate 5 --l2_clip 2.28125 --round_bound 1.  Replayed on the CPU from the candidates each
client drew, its recorded dither_seed and round_attempt -- tests/l2_cases.py in front of tests/rotate_cases.py, then
tests/round_cases.py, then tests/pack_cases.py: every client's rounded sum of squares is within the bound the server
holds, its choice is the restatement's, and final_mean is the mean of the replayed encodings bit for bit.  Without
--round_bound the same run calls no round_select and is the pipeline tests/test_l2_abides_gpu.py pins."""
import numpy as np
import pytest

import l2_cases as l2
import pack_cases as PC
import rotate_cases as R
import round_cases as RC

pytestmark = pytest.mark.gpu

N, L, F, C, P, H = 16, 1001, 7, 1.0, 2, 5
L_ROT = 1024
NORM = 2.28125


def _run(monkeypatch, extra):
    from flamingo_amd import MaskEngine
    from flamingo_amd.abides.config_flamingo import run
    from flamingo_amd.abides.flamingo import protocol
    from flamingo_amd.abides.flamingo.client_agent import SA_ClientAgent
    drew, calls = {}, []    # (client, iteration) -> (dither seed, round_attempt, rounded_sumsq, candidate batches)
    vectors, select = SA_ClientAgent.sendVectors, MaskEngine.round_select

    def round_select(self, x, frac_bits, clip, candidates, max_sumsq):
        calls.append((np.array(candidates, np.uint8).reshape(-1, 32), int(max_sumsq), np.array(x, np.float32).reshape(-1)))
        return select(self, x, frac_bits, clip, candidates, max_sumsq)

    def send_vectors(self, *a, **kw):
        del calls[:]
        out = vectors(self, *a, **kw)
        drew[(self.id, self.current_iteration)] = (self.dither_seed, self.round_attempt, self.rounded_sumsq, list(calls))
        return out

    with monkeypatch.context() as m:   # undone on the way out: a test may run twice
        m.setattr(SA_ClientAgent, "sendVectors", send_vectors)
        m.setattr(MaskEngine, "round_select", round_select)
        try:
            res = run(["-c", "flamingo", "-n", str(N), "-i", "2", "-s", "11", "-k", "--committee_size", "9",
                       "--vector_len", str(L), "--float_inputs", "7,1,sr,pack2", "--rotate", str(H), "--l2_clip", str(NORM)]
                      + extra)
            state = (protocol.round_bound(), protocol.rotated_len(), protocol.ring_len())
            keys = {it: protocol.rotation_key(it) for it in (1, 2)}
        finally:
            protocol.configure(codec=False)
    return res["server"], res["clients"], drew, state, keys


def _replayed_mean(srv, clients, drew, keys, it):
    """The rotated, clipped rows of the iteration's clients, and the check that final_mean is the mean of their
    encodings under the recorded dither seeds, bit for bit."""
    ids = srv.online_ids[it]
    ys = [l2.clip_forward(np.asarray(clients[i].input_vector, np.float32), NORM, keys[it], H)[0] for i in ids]
    enc = sum(PC.encode_packed(y, F, C, P, drew[(i, it)][0])[0].astype(np.uint64) for i, y in zip(ids, ys))
    assert int(enc.max()) < 2 ** 32 and np.array_equal(srv.results[it], enc.astype(np.uint32))
    back = R.inverse(PC.decode_packed(enc.astype(np.uint32), L_ROT, F, C, P, len(ids)), keys[it], H, L)
    assert srv.means[it].tobytes() == back.tobytes()
    return ids, ys


def test_round_bound_through_the_agents(monkeypatch, capsys):
    srv, clients, drew, state, keys = _run(monkeypatch, ["--round_bound", "1"])
    assert state == ((1.0, 4), L_ROT, L_ROT // 2)
    bound = RC.bound(NORM, F, L_ROT, 1.0)
    assert srv.round_max_sumsq == bound and (NORM * 2 ** F) ** 2 < bound < (NORM * 2 ** F + 32) ** 2
    redrawn = []
    for it in (1, 2):
        ids, ys = _replayed_mean(srv, clients, drew, keys, it)
        assert 0 < len(ids) == srv.online_counts[it] <= N
        for i, y in zip(ids, ys):
            seed, attempt, Q, batches = drew[(i, it)]
            assert len(batches) >= 1 and all(c.shape == (4, 32) and m == bound for c, m, _ in batches)
            assert all(x.tobytes() == y.tobytes() for _, _, x in batches)         # the pass saw the rotated row
            cands = np.concatenate([c for c, _, _ in batches])
            sums = [RC.sumsq(y, F, C, bytes(c)) for c in cands]
            assert attempt == RC.select(sums, bound) < len(cands), i              # the restatement's choice
            assert len(batches) == attempt // 4 + 1                              # and no batch drawn after it
            assert seed == bytes(cands[attempt]) and Q == sums[attempt] <= bound
            assert RC.sumsq(y, F, C, seed) == Q                                   # from the recorded seed alone
        redrawn.append(sum(drew[(i, it)][1] > 0 for i in ids))
    out = capsys.readouterr().out
    delta = f"rounded within Delta = sqrt({bound}) / 2^7 = {float(np.sqrt(bound)) / 128.0:g}"
    assert out.count(delta) == 2 and all(f"{delta}, {k} clients needed a redraw" in out for k in redrawn)


def test_without_round_bound_the_run_is_unchanged(monkeypatch, capsys):
    srv, clients, drew, state, keys = _run(monkeypatch, [])
    assert state == (None, L_ROT, L_ROT // 2) and srv.round_max_sumsq is None
    for it in (1, 2):
        ids, _ = _replayed_mean(srv, clients, drew, keys, it)
        assert all(drew[(i, it)][1:] == (None, None, []) and len(drew[(i, it)][0]) == 32 for i in ids)
    out = capsys.readouterr().out
    assert out.count("clients scaled to norm 2.28125") == 2 and "rounded within" not in out and "redraw" not in out
    # --round_bound 0 is the same run: the same draws, the same sums
    srv0, _, drew0, state0, _ = _run(monkeypatch, ["--round_bound", "0"])
    assert state0 == state and all(drew0[k] == drew[k] for k in drew)
    assert all(np.array_equal(srv0.results[it], srv.results[it]) and srv0.means[it].tobytes() == srv.means[it].tobytes()
               for it in (1, 2))
