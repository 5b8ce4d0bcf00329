"""The keystream kernels where their block counters carry, where the PRG's slot range ends and
where a batch crosses a workgroup, bit for bit against the CPU oracle.

* The PRG's 32-bit block counter (SeedRec.a0 / chacha_mask_add in items_kernel, prg_expand_kernel;
  ctr0 + bslot / 16 in small_round_kernel) at windows whose counters carry through bits 16..31,
  flip bit 31, and end exactly at 2^36 slots, through every items_kernel variant, pairing and
  sub-tiling, the small-round kernel, the split seed-table + aggregate form, the host
  mask_accumulate and prg_expand / prg_expand_dev.
* The range guard: one slot past 2^36, and slot offsets near 2^64 whose sum with the length wraps,
  are FLM_ERANGE on every entry point, with nothing written and the context usable afterwards.
* chacha20_xor_kernel's 64-bit counter across 2^32 and up to the last block, both nonce words set,
  lengths around one block and around one 256-block workgroup, in == out at the C ABI, n = 0.
* hash_to_curve_kernel at every message length 0..64 (b_0's SHA-256 padding moves into another
  block between len 7 and 8)."""
import numpy as np
import pytest

import ec_oracle as E
import oracle as O

pytestmark = pytest.mark.gpu

TOP = 1 << 36
L, PITCH, N = 2064, 2068, 3                  # two 1024-slot tiles and one block; a padded pitch
SENT = 0x5A5A5A5A
WINDOWS = [TOP - 2064,                       # the last lane's counter is 0xFFFFFFFF; ends at the limit
           16 * (2**31 - 64),                # bit 31 flips inside the window
           16 * (2**24 - 64),
           16 * 0xFFFEFFC0]                  # a carry through bits 16..31
KS = (5, 37)
ERANGE = r"code -4\)"


@pytest.fixture(scope="module")
def eng():
    from flamingo_amd import MaskEngine
    e = MaskEngine(0)
    yield e
    e.close()


def _inputs(K):
    g = np.random.Generator(np.random.PCG64(3600 + K))
    rows = g.integers(0, 2**32, size=(N, L), dtype=np.uint32)
    seeds = g.integers(0, 256, size=(K, 32), dtype=np.uint8)
    signs = np.where(g.random(K) < 0.5, 1, -1).astype(np.int8)
    signs[0], signs[1] = 1, -1                # both signs present
    return rows, seeds, signs


@pytest.fixture(scope="module")
def cases():
    """(K, slot0) -> host inputs, device inputs and the oracle's outputs, computed once and only read."""
    import torch
    out = {}
    for K in KS:
        rows, seeds, signs = _inputs(K)
        d_rows = torch.zeros((N, PITCH), dtype=torch.int32, device="cuda")
        d_rows[:, :L] = torch.from_numpy(rows.view(np.int32)).cuda()
        dev = (d_rows[:, :L], torch.from_numpy(seeds).cuda(), torch.from_numpy(signs).cuda())
        for slot0 in WINDOWS:
            want = O.aggregate_unmask(rows, seeds, signs, L=L, slot0=slot0)
            prg = np.stack([O.prg(s.tobytes(), L, slot0) for s in seeds])
            for a in (rows, seeds, signs, want, prg):
                a.setflags(write=False)
            out[K, slot0] = dict(rows=rows, seeds=seeds, signs=signs, dev=dev, want=want, prg=prg)
    return out


def _sentinel_out(n=PITCH):
    import torch
    return torch.full((n,), SENT, dtype=torch.int32, device="cuda")


def _check_out(out, want, what):
    import torch
    torch.cuda.synchronize()
    got = out.cpu().numpy().view(np.uint32)
    n = want.shape[0]
    assert np.array_equal(got[:n], want), (what, np.flatnonzero(got[:n] != want)[:5])
    assert np.all(got[n:] == SENT), (what, "wrote past L")


PARAMS = [pytest.param(K, s, id=f"K{K}-slot0_{s:#x}") for K in KS for s in WINDOWS]


@pytest.mark.parametrize("K,slot0", PARAMS)
def test_items_path_at_high_counters(eng, cases, K, slot0):
    """items_kernel in every variant, pairing and sub-tiling ("small" 0)."""
    c = cases[K, slot0]
    eng.set_tuning("small", 0)
    try:
        for pairing in (0, 1):
            eng.set_tuning("pairing", pairing)
            for v in (-1, 0, 1, 2, 5, 7, 8):
                eng.set_tuning("variant", v)
                for st in (0, 1, 4, 16):
                    eng.set_tuning("subtiles", st)
                    out = _sentinel_out()
                    eng.aggregate_unmask_dev(*c["dev"], out, L=L, mask_lo=0, mask_hi=L, prg_slot0=slot0)
                    _check_out(out, c["want"], (pairing, v, st))
                    assert eng.last_plan()["variant"] != 100
    finally:
        eng.set_tuning("subtiles", 0)
        eng.set_tuning("variant", -1)
        eng.set_tuning("pairing", 1)
        eng.set_tuning("small", 1)


@pytest.mark.parametrize("K,slot0", PARAMS)
def test_small_round_and_split_form_at_high_counters(eng, cases, K, slot0):
    """small_round_kernel ("small" 2), and flm_seed_table_dev + flm_aggregate_dev."""
    c = cases[K, slot0]
    eng.set_tuning("small", 2)
    try:
        out = _sentinel_out()
        eng.aggregate_unmask_dev(*c["dev"], out, L=L, mask_lo=0, mask_hi=L, prg_slot0=slot0)
        _check_out(out, c["want"], "small")
        assert eng.last_plan()["variant"] == 100
        assert eng.check_signs() == 0
    finally:
        eng.set_tuning("small", 1)
    d_rows, d_seeds, d_signs = c["dev"]
    out = _sentinel_out()
    eng.seed_table_dev(d_seeds, d_signs)
    eng.aggregate_dev(d_rows, K, out, L=L, mask_lo=0, mask_hi=L, prg_slot0=slot0)
    _check_out(out, c["want"], "split")
    assert eng.last_plan()["variant"] != 100


@pytest.mark.parametrize("K,slot0", PARAMS)
def test_host_paths_at_high_counters(eng, cases, K, slot0):
    """flm_mask_accumulate and flm_prg_expand (host pointers in and out) with the same slot0."""
    c = cases[K, slot0]
    acc = c["rows"][0].copy()
    others = c["rows"][1:].sum(axis=0, dtype=np.uint64).astype(np.uint32)
    eng.mask_accumulate(c["seeds"], c["signs"], acc, slot0=slot0)
    assert np.array_equal(acc, c["want"] - others)
    assert np.array_equal(eng.prg_expand(c["seeds"], L, slot0=slot0), c["prg"])


@pytest.mark.parametrize("waves", [1, 256])
@pytest.mark.parametrize("K,slot0", PARAMS)
def test_prg_expand_dev_at_high_counters(eng, cases, K, slot0, waves):
    import torch
    c = cases[K, slot0]
    eng.set_tuning("expand_waves", waves)
    try:
        out = torch.full((K, PITCH), SENT, dtype=torch.int32, device="cuda")
        eng.prg_expand_dev(c["dev"][1], out, L, slot0=slot0)
        torch.cuda.synchronize()
        got = out.cpu().numpy().view(np.uint32)
        assert np.array_equal(got[:, :L], c["prg"]), np.argwhere(got[:, :L] != c["prg"])[:5]
        assert np.all(got[:, L:] == SENT), "wrote past L"
        assert eng.last_plan()["variant"] == 101
    finally:
        eng.set_tuning("expand_waves", 128)


@pytest.mark.parametrize("small", [0, 2])
@pytest.mark.parametrize("K", KS)
def test_clipped_window_ends_at_the_limit(eng, K, small):
    """prg_slot0 + L > 2^36 but prg_slot0 + mask_hi == 2^36: the header's rule is on the window."""
    import torch
    Lc, lo, hi, slot0 = 4096, 1024, 2064, TOP - 2064
    g = np.random.Generator(np.random.PCG64(4800 + K))
    rows = g.integers(0, 2**32, size=(N, Lc), dtype=np.uint32)
    _, seeds, signs = _inputs(K)
    want = rows.sum(axis=0, dtype=np.uint64).astype(np.uint32)
    want[lo:hi] += O.aggregate_unmask(np.zeros((0, 1), np.uint32), seeds, signs, L=hi - lo, slot0=slot0 + lo)
    d_rows = torch.zeros((N, Lc + 4), dtype=torch.int32, device="cuda")
    d_rows[:, :Lc] = torch.from_numpy(rows.view(np.int32)).cuda()
    eng.set_tuning("small", small)
    try:
        out = _sentinel_out(Lc + 4)
        eng.aggregate_unmask_dev(d_rows[:, :Lc], torch.from_numpy(seeds).cuda(), torch.from_numpy(signs).cuda(), out,
                                 L=Lc, mask_lo=lo, mask_hi=hi, prg_slot0=slot0)
        _check_out(out, want, small)
        assert (eng.last_plan()["variant"] == 100) == (small == 2)
    finally:
        eng.set_tuning("small", 1)


@pytest.mark.parametrize("slot0", [TOP - 2048, 2**64 - 16, 2**64 - 2064],
                         ids=["one_block_past_2_36", "2_64_minus_16", "2_64_minus_2064"])
def test_windows_past_the_limit_are_refused(eng, cases, slot0):
    """FLM_ERANGE from every entry point that takes a slot offset, before anything is enqueued: the
    outputs keep their sentinel, and the context runs a valid round afterwards.  For the two offsets
    near 2^64 the 64-bit sum slot0 + 2064 wraps to 2048 and to 0."""
    import torch
    K = 5
    c = cases[K, WINDOWS[0]]
    d_rows, d_seeds, d_signs = c["dev"]
    for small in (0, 2):
        eng.set_tuning("small", small)
        try:
            out = _sentinel_out()
            with pytest.raises(RuntimeError, match=ERANGE):
                eng.aggregate_unmask_dev(d_rows, d_seeds, d_signs, out, L=L, mask_lo=0, mask_hi=L, prg_slot0=slot0)
            torch.cuda.synchronize()
            assert bool((out == SENT).all().item())
        finally:
            eng.set_tuning("small", 1)
    eng.seed_table_dev(d_seeds, d_signs)
    out = _sentinel_out()
    with pytest.raises(RuntimeError, match=ERANGE):
        eng.aggregate_dev(d_rows, K, out, L=L, mask_lo=0, mask_hi=L, prg_slot0=slot0)
    exp = torch.full((K, PITCH), SENT, dtype=torch.int32, device="cuda")
    with pytest.raises(RuntimeError, match=ERANGE):
        eng.prg_expand_dev(d_seeds, exp, L, slot0=slot0)
    torch.cuda.synchronize()
    assert bool((out == SENT).all().item()) and bool((exp == SENT).all().item())
    with pytest.raises(RuntimeError, match=ERANGE):
        eng.prg_expand(c["seeds"], L, slot0=slot0)
    acc = np.full(L, SENT, np.uint32)
    with pytest.raises(RuntimeError, match=ERANGE):
        eng.mask_accumulate(c["seeds"], c["signs"], acc, slot0=slot0)
    assert np.all(acc == SENT)
    # the context still works
    out = _sentinel_out()
    eng.aggregate_unmask_dev(d_rows, d_seeds, d_signs, out, L=L, mask_lo=0, mask_hi=L, prg_slot0=WINDOWS[0])
    _check_out(out, c["want"], "after the refusals")


# ------------------------------------------------------------------ byte keystream
CHA_NONCE = bytes.fromhex("0102030405060708")
CHA_KEYS = [bytes(range(32)), bytes(np.random.Generator(np.random.PCG64(77)).integers(0, 256, 32, dtype=np.uint8))]
CHA_LENS = (1, 63, 64, 65, 127, 16383, 16384, 16385, 30720)   # one block; one 256-block workgroup; choose_committee's
CHA_DATA = bytes(np.random.Generator(np.random.PCG64(78)).integers(0, 256, 30720, dtype=np.uint8))


@pytest.mark.parametrize("counter", [2**32 - 2, 2**32 - 256, 2**40 - 1], ids=["2_32-2", "2_32-256", "2_40-1"])
@pytest.mark.parametrize("ki", [0, 1])
def test_chacha20_counter_carries_into_x13(eng, ki, counter):
    """x12 carries into x13 inside a workgroup (2^32 - 2), at the end of the first workgroup
    (2^32 - 256 with more than 16384 bytes), and x13 alone counts (2^40 - 1)."""
    key = CHA_KEYS[ki]
    for n in CHA_LENS:
        got = eng.chacha20_encrypt(key, CHA_DATA[:n], CHA_NONCE, counter=counter)
        assert got == O.chacha20_encrypt(key, CHA_DATA[:n], CHA_NONCE, counter=counter), (n, counter)


@pytest.mark.parametrize("ki", [0, 1])
def test_chacha20_ends_at_the_last_block(eng, ki):
    """counter = 2^64 - 4 with exactly four blocks: the last one is block 2^64 - 1."""
    key, data = CHA_KEYS[ki], CHA_DATA[:256]
    assert eng.chacha20_encrypt(key, data, CHA_NONCE, counter=2**64 - 4) == \
        O.chacha20_encrypt(key, data, CHA_NONCE, counter=2**64 - 4)


def test_chacha20_in_place_and_empty_at_the_abi(eng):
    """flm_chacha20_xor with in == out, and n = 0: returns 0 and leaves out alone."""
    from flamingo_amd._lib import p_u8
    key, counter, n = CHA_KEYS[1], 2**32 - 2, 16385
    k, nn = np.frombuffer(key, np.uint8).copy(), np.frombuffer(CHA_NONCE, np.uint8).copy()
    buf = np.frombuffer(CHA_DATA[:n], np.uint8).copy()
    assert eng.lib.flm_chacha20_xor(eng.ctx, p_u8(k), p_u8(nn), counter, p_u8(buf), p_u8(buf), n) == 0
    assert buf.tobytes() == O.chacha20_encrypt(key, CHA_DATA[:n], CHA_NONCE, counter=counter)
    src, dst = np.frombuffer(CHA_DATA[:64], np.uint8).copy(), np.full(64, 0xA5, np.uint8)
    assert eng.lib.flm_chacha20_xor(eng.ctx, p_u8(k), p_u8(nn), counter, p_u8(src), p_u8(dst), 0) == 0
    assert np.all(dst == 0xA5)
    assert eng.chacha20_encrypt(key, b"", CHA_NONCE, counter=counter) == b""


# ------------------------------------------------------------------ hash to curve
@pytest.mark.parametrize("kind", ["random", "ff"])
def test_hash_to_curve_every_message_length(eng, kind):
    """One batch with a message of every length 0..64 (65 lanes: the SHA-256 padding of
    Z_pad || msg || ... spills into another block between len 7 and 8)."""
    g = np.random.Generator(np.random.PCG64(65))
    msgs = [bytes(g.integers(0, 256, ln, dtype=np.uint8)) if kind == "random" else b"\xff" * ln for ln in range(65)]
    out, fl = eng.hash_to_curve_wire(msgs)
    assert not fl.any()
    for m, row in zip(msgs, out):
        assert row.tobytes() == E.wire(E.hash_str_to_curve(m)), len(m)
