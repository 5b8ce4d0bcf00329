"""Host-side handle on the MI355X engine (libflamingo_hip.so).

``MaskEngine`` owns one C-ABI context bound to one GPU (one process per GPU).
Its methods are the calls the drop-in agents make in place of the reference's
numpy/pycryptodomex loops:

* ``aggregate_unmask`` -- SA_ServiceAgent.report_process partial sum
  (agent/flamingo/SA_ServiceAgent.py:346-350) + reconstruction_process unmask
  and combine (:529-540, :587-605).
* ``client_mask`` -- SA_ClientAgent.sendVectors mask composition
  (agent/flamingo/SA_ClientAgent.py:246-324), batched over clients.
* ``prg_expand`` / ``prg`` -- the PRG idiom ChaCha20(seed).encrypt(b"abcd"*L)
  viewed as uint32 (SA_ClientAgent.py:248-250).
* ``chacha20_encrypt`` -- ChaCha20.new(key, nonce).encrypt(data) for the
  PRF/PRG calls of util/param.py:44-46, 63-76.
* ``shamir_deal`` / ``aes_gcm_xor_wire`` -- the clients' dealing and AES-GCM sealing of their
  m_i shares (SA_ClientAgent.py:218-220, 227-244) and the committee's opening of them
  (:402-420), batched over clients.
* ``ecdsa_verify`` / ``ecdsa_verify_wire`` -- ECDSA P-256 verification of a batch of signatures: the
  committee's check of the server's and the members' signatures (SA_ClientAgent.py:387).
* ``*_dev`` -- the same on device-resident torch tensors (bench, multi-GPU).

Errors surface as RuntimeError with the library's message, like the
reference's own guards (SA_ServiceAgent.py:349, 502).
"""
from __future__ import annotations

import ctypes
import math

import numpy as np

from . import _lib
from ._lib import p_f32, p_f64, p_i8, p_i64, p_u8, p_u32, p_u64

NONCE = b"\x00" * 8


def _seeds_array(seeds) -> np.ndarray:
    if isinstance(seeds, (list, tuple)):
        if len(seeds) == 0:
            return np.zeros((0, 32), np.uint8)
        if isinstance(seeds[0], (bytes, bytearray)):
            if any(len(s) != 32 for s in seeds):
                raise RuntimeError("every seed must be 32 bytes")
            return np.frombuffer(b"".join(bytes(s) for s in seeds), dtype=np.uint8).reshape(-1, 32).copy()
    a = np.ascontiguousarray(seeds, dtype=np.uint8)
    if a.size % 32:
        raise RuntimeError("seeds must be K x 32 bytes")
    return a.reshape(-1, 32)


def _signs_array(signs, K: int) -> np.ndarray:
    s = np.ascontiguousarray(signs, dtype=np.int8).reshape(-1)
    if s.shape[0] != K:
        raise RuntimeError(f"{s.shape[0]} signs for {K} seeds")
    return s


def _need(cond: bool, msg: str):
    if not cond:
        raise RuntimeError(msg)


def _dev_bytes(t, name: str, cols: int, rows: int, dtype_bytes: int = 1):
    """A contiguous CUDA tensor of >= rows x cols elements of dtype_bytes each (the kernels index it flat)."""
    _need(t is not None and t.is_cuda and t.is_contiguous() and t.element_size() == dtype_bytes,
          f"{name} must be a contiguous CUDA tensor of {dtype_bytes}-byte elements")
    _need(t.numel() >= rows * cols and (cols == 1 or t.shape[-1] == cols),
          f"{name} must hold >= {rows} x {cols} elements, got {tuple(t.shape)}")


def _vp(t) -> ctypes.c_void_p:
    """A CUDA tensor's address for a *_dev call; None: a NULL pointer."""
    return ctypes.c_void_p(t.data_ptr() if t is not None else None)


def _dev_vector(name: str, t, n: int, kind, label: str | None = None, flat: bool = False):
    """t is None or a contiguous (>= n,) tensor of dtype `kind` (an int: of that element size), which the message
    names by `label`, or as the dtype prints; flat: of any shape, >= n elements."""
    if t is None:
        return
    fits = t.numel() >= n if flat else t.dim() == 1 and t.shape[0] >= n
    if not (fits and (t.element_size() if isinstance(kind, int) else t.dtype) == kind and t.is_contiguous()):
        raise RuntimeError(f"{name} must hold >= {n} contiguous {label or kind} words" if flat else
                           f"{name} must be a contiguous (>= {n},) {label or kind} tensor")


def _float_rows_array(x) -> tuple:
    """x (N, L) or (L,) as a contiguous (N, L) float32 array, and whether it came as one row."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    one = x.ndim == 1
    if one:
        x = x[None, :]
    if x.ndim != 2:
        raise RuntimeError("x must be (N, L) or (L,)")
    return x, one


def _dev_rows(rows, L: int) -> int:
    """Row pitch (elements) of an (N, >= L) 32-bit CUDA tensor whose rows may be a strided view."""
    _need(rows.is_cuda and rows.dim() == 2 and rows.element_size() == 4, "rows must be a 2-D 32-bit CUDA tensor")
    _need(rows.shape[1] <= 1 or rows.stride(1) == 1, "rows must be contiguous along a row")
    pitch = rows.stride(0) if rows.shape[0] > 1 else rows.shape[1]
    _need(rows.shape[1] >= L and pitch >= rows.shape[1], f"rows must be (N, >= {L}), got {tuple(rows.shape)}")
    return pitch


def _client_seeds(seg, signs, seeds_dev):
    """seg and signs of a client_*_dev call as the C side reads them, with N and K = seg[-1].  The C side
    reads signs[0..K) from the host array and indexes the K device seeds by seg, 32 bytes apart: all
    three are checked here, where the shapes are known."""
    seg = np.ascontiguousarray(seg, dtype=np.int64)
    N = seg.shape[0] - 1
    signs = np.ascontiguousarray(signs, dtype=np.int8)
    K = int(seg[-1]) if N >= 0 else 0
    if N < 0 or seg[0] != 0 or np.any(np.diff(seg) < 0):
        raise RuntimeError("seg must be non-decreasing from 0")
    if signs.ndim != 1 or signs.shape[0] != K:
        raise RuntimeError(f"{signs.shape[0] if signs.ndim else 0} signs for seg[-1] = {K} seeds")
    if K and (seeds_dev.dim() != 2 or seeds_dev.shape[1] != 32 or seeds_dev.element_size() != 1
              or seeds_dev.shape[0] < K or not seeds_dev.is_contiguous()):
        raise RuntimeError(f"seeds_dev must be a contiguous (>= {K}, 32) uint8 tensor, got {tuple(seeds_dev.shape)}")
    return seg, signs, N, K


class MaskEngine:
    """One GPU's mask-and-aggregate engine (a flm_ctx)."""

    def __init__(self, device: int = 0, _ctx=None):
        self.lib = _lib.load()
        self.device = device
        self._owned = _ctx is None
        if _ctx is not None:                 # a context owned by a DeviceGroup
            self.ctx = ctypes.c_void_p(_ctx)
            return
        ctx = ctypes.c_void_p()
        rc = self.lib.flm_init(ctypes.byref(ctx), device)
        if rc != 0:
            raise RuntimeError(f"flm_init(device={device}) failed: {self.lib.flm_last_error(None).decode()}")
        self.ctx = ctx

    # ------------------------------------------------------------ plumbing
    def close(self):
        if not getattr(self, "_owned", True):
            self.ctx = None
            return
        if getattr(self, "ctx", None) is not None and self.ctx.value:
            for st in self.__dict__.pop("_cu_streams", {}).values():
                st.synchronize()
                self.lib.flm_stream_destroy(self.ctx, ctypes.c_void_p(st.cuda_stream))
            self.lib.flm_free(self.ctx)
            self.ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _check(self, rc: int, what: str):
        if rc != 0:
            raise RuntimeError(f"{what}: {self.lib.flm_last_error(self.ctx).decode()} (code {rc})")

    def set_tuning(self, key: str, value: int):
        """A/B knobs (flm_set_tuning, include/flamingo_hip.h): variant, subtiles, pairing, ..."""
        self._check(self.lib.flm_set_tuning(self.ctx, key.encode(), int(value)), f"flm_set_tuning({key})")

    def get_tuning(self, key: str) -> int:
        """The context's current value of `key` (flm_get_tuning): also what another wrapper of the
        same flm_ctx (DeviceGroup engines, a direct flm_set_tuning call) set."""
        v = ctypes.c_int()
        self._check(self.lib.flm_get_tuning(self.ctx, key.encode(), ctypes.byref(v)), f"flm_get_tuning({key})")
        return v.value

    def last_plan(self) -> dict:
        v = [ctypes.c_int() for _ in range(4)]
        self.lib.flm_last_plan(self.ctx, *[ctypes.byref(x) for x in v])
        return {"items": v[0].value, "tile_slots": v[1].value, "atomics": v[2].value, "variant": v[3].value}

    def cu_count(self) -> int:
        n = ctypes.c_int()
        self._check(self.lib.flm_cu_count(self.ctx, ctypes.byref(n)), "flm_cu_count")
        return n.value

    def cu_stream(self, cus):
        """A torch ExternalStream whose kernels run only on the logical CUs in `cus`
        (flm_stream_create_cu_mask).  Cached per CU set and owned by the engine:
        destroyed by close() after a device synchronize.  Never record_stream() a
        tensor on it (the caching allocator would touch the stream after close)."""
        import torch
        cus = tuple(sorted(set(int(c) for c in cus)))
        if not cus:
            raise ValueError("cu_stream: empty CU set")
        cache = self.__dict__.setdefault("_cu_streams", {})
        if cus in cache:
            return cache[cus]
        words = np.zeros((max(cus) // 32) + 1, np.uint32)
        for c in cus:
            words[c // 32] |= np.uint32(1 << (c % 32))
        h = ctypes.c_void_p()
        self._check(self.lib.flm_stream_create_cu_mask(self.ctx, words.ctypes.data_as(ctypes.c_void_p), len(words),
                                                        ctypes.byref(h)), "flm_stream_create_cu_mask")
        cache[cus] = torch.cuda.ExternalStream(h.value, device=torch.device("cuda", self.device))
        return cache[cus]

    # ----------------------------------------------- RCCL (one process per GPU)
    def comm_init(self, n_ranks: int, rank: int, unique_id: bytes):
        """Attach an RCCL communicator (flm_comm_init_rank; collective over all ranks)."""
        uid = (ctypes.c_uint8 * 128).from_buffer_copy(bytes(unique_id))
        self._check(self.lib.flm_comm_init_rank(self.ctx, int(n_ranks), int(rank), uid), "flm_comm_init_rank")

    def comm_destroy(self):
        """Synchronise the device, then finalize + destroy the attached RCCL communicator
        (flm_comm_destroy; a no-op without one).  distributed.shutdown calls this on every rank
        before torch.distributed's process group is destroyed."""
        if getattr(self, "ctx", None) is not None and self.ctx.value:
            self._check(self.lib.flm_comm_destroy(self.ctx), "flm_comm_destroy")

    def comm_size(self):
        """(n_ranks, rank) of the attached communicator, (1, 0) without one."""
        n, r = ctypes.c_int(), ctypes.c_int()
        self.lib.flm_comm_size(self.ctx, ctypes.byref(n), ctypes.byref(r))
        return n.value, r.value

    def has_comm(self) -> bool:
        """True when an RCCL communicator is attached (flm_comm_size returns 0; 1 = none)."""
        n, r = ctypes.c_int(), ctypes.c_int()
        return self.lib.flm_comm_size(self.ctx, ctypes.byref(n), ctypes.byref(r)) == 0

    def reduce_scatter_dev(self, send, recv, recv_words: int | None = None, stream=None):
        """recv[:recv_words] = this rank's slice of sum_ranks(send) as uint32 (ncclUint32, ncclSum)."""
        n = int(recv.numel() if recv_words is None else recv_words)
        if send.numel() < n * self.comm_size()[0] or recv.numel() < n or send.element_size() != 4:
            raise RuntimeError("reduce_scatter_dev: send must hold n_ranks * recv_words 32-bit words")
        self._check(self.lib.flm_reduce_scatter_dev(self.ctx, send.data_ptr(), recv.data_ptr(), n,
                                                    self._stream_handle(stream)), "flm_reduce_scatter_dev")
        return recv

    def all_gather_dev(self, send, recv, stream=None):
        """recv = concat over ranks of send's bytes (ncclAllGather, ncclUint8)."""
        nb = send.numel() * send.element_size()
        if recv.numel() * recv.element_size() < nb * self.comm_size()[0]:
            raise RuntimeError("all_gather_dev: recv too small")
        self._check(self.lib.flm_all_gather_dev(self.ctx, send.data_ptr(), recv.data_ptr(), nb,
                                                self._stream_handle(stream)), "flm_all_gather_dev")
        return recv

    # -------------------------------------------------------- host arrays
    def aggregate_unmask(self, vectors, seeds, signs, L: int | None = None) -> np.ndarray:
        """sum(vectors) + sum_k signs[k]*PRG(seeds[k]) mod 2^32 (host in, host out).

        vectors: a list of uint32 arrays (the VECTOR bodies) or an (N, L) array."""
        if isinstance(vectors, np.ndarray) and vectors.ndim == 2:
            rows = [np.ascontiguousarray(vectors[i], dtype=np.uint32) for i in range(vectors.shape[0])]
        else:
            rows = [np.ascontiguousarray(v, dtype=np.uint32) for v in vectors]
        if L is None:
            if not rows:
                raise RuntimeError("L is required when there are no vectors")
            L = rows[0].shape[0]
        for v in rows:
            if v.shape[0] != L:
                raise RuntimeError("Client sends vector of incorrect length.")  # SA_ServiceAgent.py:348-349
        seeds = _seeds_array(seeds)
        signs = _signs_array(signs, seeds.shape[0])
        out = np.empty(L, dtype=np.uint32)
        ptrs = (_lib._u32p * max(1, len(rows)))(*[p_u32(v) for v in rows])
        rc = self.lib.flm_aggregate_unmask(self.ctx, ptrs, len(rows), p_u8(seeds), p_i8(signs), seeds.shape[0],
                                           L, p_u32(out))
        self._check(rc, "flm_aggregate_unmask")
        return out

    def client_mask(self, seg, seeds, signs, L: int, x: np.ndarray | None = None) -> np.ndarray:
        """y_i = x_i (or ones) + sum_{k in seg i} signs[k]*PRG(seeds[k]); returns (N, L) uint32."""
        seg = np.ascontiguousarray(seg, dtype=np.int64)
        N = seg.shape[0] - 1
        seeds = _seeds_array(seeds)
        signs = _signs_array(signs, seeds.shape[0])
        if seg[-1] != seeds.shape[0]:
            raise RuntimeError("seg[-1] must equal the number of seeds")
        out = np.empty((N, L), dtype=np.uint32)
        xp = None
        if x is not None:
            x = np.ascontiguousarray(x, dtype=np.uint32)
            if x.shape != (N, L):
                raise RuntimeError("x must be (N, L)")
            xp = p_u32(x)
        rc = self.lib.flm_client_mask(self.ctx, xp, N, p_i64(seg), p_u8(seeds), p_i8(signs), L, p_u32(out))
        self._check(rc, "flm_client_mask")
        return out

    # ------------------------------------------------- fixed-point codec
    def codec_check(self, frac_bits: int, clip: float, n_clients: int = 1, pack: int = 1, noise_bits: int = 0, L: int = 0):
        """Raise unless n_clients updates of magnitude <= clip fit the 32-bit ring at frac_bits
        (flm_codec_check: n * ceil(clip * 2^frac_bits) <= 2^31 - 1); no device call.  pack = 2 or 4: the
        packed codec's rule instead (flm_codec_check_packed: n * 2 ceil(clip * 2^frac_bits) <= 2^(32/pack) - 1).
        noise_bits > 0: the rule with every client's binomial noise share (flm_codec_check_noise: the worst case,
        ceil(clip * 2^frac_bits) + noise_bits / 2 in the bound's place, and for L > 0 parameters the noise
        stream's length rule ceil(noise_bits / 32) * ceil(L / 16) <= 2^32).  flm_codec_check_noise is all three:
        without noise it is the rule of the pack."""
        rc = self.lib.flm_codec_check_noise(int(frac_bits), float(clip), int(pack), int(noise_bits), int(n_clients), int(L))
        self._check(rc, "flm_codec_check_noise")

    def _encode_mask(self, fn: str, codec, seg, seeds, signs, L: int, x, frac_bits: int, clip: float, pack: int, dither,
                     noise, return_clipped: bool):
        """The host form of the three encode calls.  codec(dither, noise): the arguments of `fn` between clip and
        out, which is where the three differ."""
        seg = np.ascontiguousarray(seg, dtype=np.int64)
        N = seg.shape[0] - 1
        seeds = _seeds_array(seeds)
        signs = _signs_array(signs, seeds.shape[0])
        if seg[-1] != seeds.shape[0]:
            raise RuntimeError("seg[-1] must equal the number of seeds")
        if x is None:
            raise RuntimeError("x is required")
        x = np.ascontiguousarray(x, dtype=np.float32)
        if x.shape != (N, L):
            raise RuntimeError("x must be (N, L)")
        ptrs = []
        for name, s in (("dither", dither), ("noise", noise)):
            if s is not None:
                s = _seeds_array(s)
                if s.shape[0] != N:
                    raise RuntimeError(f"one 32-byte {name} seed per client")
            ptrs.append(p_u8(s) if s is not None else None)
        out = np.empty((N, -(-L // pack) if pack > 0 else 0), dtype=np.uint32)
        clipped = np.zeros(N, dtype=np.uint32)
        rc = getattr(self.lib, fn)(self.ctx, p_f32(x), N, p_i64(seg), p_u8(seeds), p_i8(signs), L, int(frac_bits),
                                   float(clip), *codec(*ptrs), p_u32(out), p_u32(clipped) if return_clipped else None)
        self._check(rc, fn)
        return (out, clipped) if return_clipped else out

    def client_encode_mask(self, seg, seeds, signs, L: int, x: np.ndarray, frac_bits: int, clip: float, dither=None,
                           return_clipped: bool = False):
        """y_i = encode(x_i) + sum_{k in seg i} signs[k]*PRG(seeds[k]) for float32 x (N, L); (N, L) uint32.

        dither: N 32-byte seeds for stochastic rounding, None for nearest-even.  With
        return_clipped, also the (N,) uint32 counts of elements that were NaN or beyond +-clip."""
        return self._encode_mask("flm_client_encode_mask", lambda d, z: (d,), seg, seeds, signs, L, x, frac_bits, clip, 1,
                                 dither, None, return_clipped)

    def client_encode_pack_mask(self, seg, seeds, signs, L: int, x: np.ndarray, frac_bits: int, clip: float,
                                pack: int, dither=None, return_clipped: bool = False):
        """client_encode_mask with `pack` (2 or 4) parameters per ring word: float32 x (N, L) in,
        (N, ceil(L / pack)) uint32 out; field j of word l' is encode(x[pack l' + j]) + ceil(clip 2^frac_bits).
        The dither stream is indexed by parameter.  flm_client_encode_pack_mask."""
        pack = int(pack)
        return self._encode_mask("flm_client_encode_pack_mask", lambda d, z: (pack, d), seg, seeds, signs, L, x, frac_bits,
                                 clip, pack, dither, None, return_clipped)

    def client_encode_noise_mask(self, seg, seeds, signs, L: int, x: np.ndarray, frac_bits: int, clip: float,
                                 pack: int = 1, dither=None, noise_bits: int = 0, noise=None,
                                 return_clipped: bool = False):
        """client_encode_mask (pack = 1) or client_encode_pack_mask (2, 4) with every client's share of
        distributed-DP noise added inside the kernel: Z = (popcount of noise_bits coins of PRG(noise_i)) -
        noise_bits / 2 on each parameter's quantised value.  noise: N 32-byte seeds, secret and fresh per
        iteration.  noise_bits = 0: the calls without noise, bit for bit (noise is ignored).
        flm_client_encode_noise_mask."""
        pack = int(pack)
        return self._encode_mask("flm_client_encode_noise_mask", lambda d, z: (pack, d, int(noise_bits), z), seg, seeds,
                                 signs, L, x, frac_bits, clip, pack, dither, noise, return_clipped)

    def codec_check_gauss(self, frac_bits: int, clip: float, tail: int, n_clients: int = 1, pack: int = 1, L: int = 0):
        """codec_check with every client's table-sampled noise share in [-tail, tail] (flm_codec_check_gauss: tail in
        1..512, ceil(clip * 2^frac_bits) + tail in the bound's place, and for L > 0 parameters the noise stream's
        length rule 2 * ceil(L / 16) <= 2^32); no device call."""
        rc = self.lib.flm_codec_check_gauss(int(frac_bits), float(clip), int(pack), int(tail), int(n_clients), int(L))
        self._check(rc, "flm_codec_check_gauss")

    def client_encode_gauss_mask(self, seg, seeds, signs, L: int, x: np.ndarray, frac_bits: int, clip: float, table,
                                 noise, pack: int = 1, dither=None, return_clipped: bool = False):
        """client_encode_noise_mask with the noise share sampled from a cumulative table (flamingo_amd.dgauss.table):
        table 2 * tail uint64 entries, non-decreasing; Z = #{j : table[j] <= u} - tail on each parameter's quantised
        value, u the parameter's 64-bit draw of PRG(noise_i).  noise: N 32-byte seeds, secret and fresh per
        iteration.  Rows decode as rows of client_encode_noise_mask with noise_bits = 2 * tail.
        flm_client_encode_gauss_mask."""
        pack = int(pack)
        table = np.ascontiguousarray(table, dtype=np.uint64)
        if table.ndim != 1 or table.shape[0] % 2:
            raise RuntimeError("table must hold 2 * tail uint64 entries")
        tail = table.shape[0] // 2
        return self._encode_mask("flm_client_encode_gauss_mask", lambda d, z: (pack, d, tail, p_u64(table), z), seg, seeds,
                                 signs, L, x, frac_bits, clip, pack, dither, noise, return_clipped)

    def decode_unpack(self, total: np.ndarray, L: int, frac_bits: int, clip: float, pack: int, count: int = 1,
                      noise_bits: int = 0) -> np.ndarray:
        """The L float32 means of `count` contributors held in the ceil(L / pack) summed packed words `total`:
        field - count ceil(clip 2^frac_bits), over count 2^frac_bits.  noise_bits > 0: rows of
        client_encode_noise_mask, whose bias is ceil(clip 2^frac_bits) + noise_bits / 2.  flm_decode_unpack_noise,
        which without noise is flm_decode_unpack."""
        total = np.ascontiguousarray(total, dtype=np.uint32)
        pack = int(pack)
        if total.ndim != 1 or (pack > 0 and total.shape[0] != -(-L // pack)):
            raise RuntimeError("total must be a vector of ceil(L / pack) words")
        out = np.empty(L, dtype=np.float32)
        rc = self.lib.flm_decode_unpack_noise(self.ctx, p_u32(total), L, int(frac_bits), float(clip), pack,
                                              int(noise_bits), int(count), p_f32(out))
        self._check(rc, "flm_decode_unpack_noise")
        return out

    def codec_check_modular(self, frac_bits: int, clip: float, n_clients: int = 1, pack: int = 2, noise_bits: int = 0):
        """Raise unless a packed sum over n_clients can be decoded modulo the field (flm_codec_check_modular): pack 2 or
        4, one contributor's field fits (2 (ceil(clip * 2^frac_bits) + noise_bits / 2) <= 2^(32/pack) - 1) and
        n_clients <= 2^31 - 1; n_clients times the bias is not bounded.  The table mode of the noise passes noise_bits =
        2 * tail.  No device call."""
        rc = self.lib.flm_codec_check_modular(int(frac_bits), float(clip), int(pack), int(noise_bits), int(n_clients))
        if rc != 0:     # a call without a context: its text is the library's, not this context's
            raise RuntimeError(f"flm_codec_check_modular: {self.lib.flm_last_error(None).decode()} (code {rc})")

    def decode_unpack_mod(self, total: np.ndarray, L: int, frac_bits: int, clip: float, pack: int, count: int = 1,
                          noise_bits: int = 0, guard: int = 1, stats: bool = True):
        """decode_unpack of a sum taken modulo the field: every field of `total` is read as a residue mod 2^(32/pack),
        centred into [-H, H - 1], H = 2^(32/pack - 1), and its carry followed into the field above
        (flm_decode_unpack_mod).  Returns (the L float32 means, (near, max_abs)): near the number of parameters whose
        centred sum has magnitude >= guard (an integer in 1..H), max_abs the largest magnitude; stats=False asks for
        neither and returns (means, None)."""
        total = np.ascontiguousarray(total, dtype=np.uint32)
        pack = int(pack)
        if total.ndim != 1 or (pack > 0 and total.shape[0] != -(-L // pack)):
            raise RuntimeError("total must be a vector of ceil(L / pack) words")
        out = np.empty(L, dtype=np.float32)
        st = np.zeros(2, dtype=np.uint32)
        rc = self.lib.flm_decode_unpack_mod(self.ctx, p_u32(total), L, int(frac_bits), float(clip), pack, int(noise_bits),
                                            int(count), int(guard), p_f32(out), p_u32(st) if stats else None)
        self._check(rc, "flm_decode_unpack_mod")
        return out, ((int(st[0]), int(st[1])) if stats else None)

    # ------------------------------------- randomised block Hadamard rotation
    def rotate_check(self, L: int, log2_block: int) -> int:
        """L_rot = round_up(L, 2^log2_block), the length a row of L parameters has once rotated; raises for
        log2_block outside 4..12, L = 0, or a row whose sign stream would pass the PRG's range.  No device call.
        flm_rotate_check."""
        L_rot = ctypes.c_uint64(0)
        self._check(self.lib.flm_rotate_check(int(L), int(log2_block), ctypes.byref(L_rot)), "flm_rotate_check")
        return int(L_rot.value)

    def rotate(self, x: np.ndarray, key, log2_block: int, inverse: bool = False, L: int | None = None,
               return_nonfinite: bool = False, clip_norm: float | None = None):
        """The randomised block Hadamard rotation of float32 rows under the 32-byte public `key` (flm_rotate).
        Forward: x (N, L) or (L,) in, (N, L_rot) out, L_rot = round_up(L, 2^log2_block); non-finite inputs become
        +0.0 and, with return_nonfinite, are counted per row.  Inverse: x (N, L_rot) in and the first L parameters
        out (L is required: the rows' length before the rotation).
        clip_norm = C (forward only): every row is first scaled to an L2 norm of at most C, in the same pass
        (flm_rotate_clip), and the factors (N,) float32 and sums of squares (N,) float64 are returned behind the
        other results: (out, factors, sumsq), or (out, nonfinite, factors, sumsq)."""
        x, one = _float_rows_array(x)
        N = x.shape[0]
        if not inverse:
            if L is not None and int(L) != x.shape[1]:
                raise RuntimeError("forward: L is the row length of x")
            L = x.shape[1]
        elif L is None:
            raise RuntimeError("inverse: L, the rows' length before the rotation, is required")
        L = int(L)
        L_rot = self.rotate_check(L, log2_block)
        if inverse and x.shape[1] != L_rot:
            raise RuntimeError(f"inverse: x must hold rows of L_rot = {L_rot} floats")
        if inverse and return_nonfinite:
            raise RuntimeError("the inverse rotation counts nothing")
        if inverse and clip_norm is not None:
            raise RuntimeError("the inverse rotation clips nothing")
        key = _seeds_array([key] if isinstance(key, (bytes, bytearray)) else key)
        if key.shape[0] != 1:
            raise RuntimeError("one 32-byte rotation key")
        out = np.empty((N, L if inverse else L_rot), dtype=np.float32)
        nonfinite = np.zeros(N, dtype=np.uint32)
        counts = p_u32(nonfinite) if return_nonfinite else None
        clipped = ()
        if clip_norm is not None:
            self.l2_clip_check(L, clip_norm, N)
            clipped = (np.empty(N, dtype=np.float32), np.empty(N, dtype=np.float64))
            rc = self.lib.flm_rotate_clip(self.ctx, p_f32(x), N, L, int(log2_block), p_u8(key), float(clip_norm), p_f32(out),
                                          counts, p_f32(clipped[0]), p_f64(clipped[1]))
            self._check(rc, "flm_rotate_clip")
        else:
            rc = self.lib.flm_rotate(self.ctx, p_f32(x), N, L, int(log2_block), p_u8(key), int(bool(inverse)), p_f32(out),
                                     counts)
            self._check(rc, "flm_rotate")
        res = (out[0] if one else out,) + ((nonfinite,) if return_nonfinite else ()) + clipped
        return res if len(res) > 1 else res[0]

    # ------------------------------------- L2 clip in front of the rotation
    def l2_clip_check(self, L: int, clip_norm: float, N: int = 1) -> int:
        """The doubles of work space flm_l2_factors_dev needs for N rows of L parameters, N ceil(L / 4096); raises for
        L = 0, N < 1, a clip_norm that is not finite and positive, or more tiles than one launch takes.  No device
        call.  flm_l2_clip_check."""
        work = ctypes.c_uint64(0)
        self._check(self.lib.flm_l2_clip_check(int(L), float(clip_norm), int(N), ctypes.byref(work)), "flm_l2_clip_check")
        return int(work.value)

    def l2_clip(self, x: np.ndarray, clip_norm: float):
        """x (N, L) or (L,) float32 scaled row by row to an L2 norm of at most clip_norm (flm_l2_clip):
        (out, factors (N,) float32, sumsq (N,) float64), out = x factors[row], factors = min(1, clip_norm /
        sqrt(sumsq)) by the rule of include/flamingo_hip.h; non-finite inputs count as 0 in sumsq and are scaled
        like any other (NaN stays NaN)."""
        x, one = _float_rows_array(x)
        N, L = x.shape
        self.l2_clip_check(L, clip_norm, N)
        out = np.empty((N, L), dtype=np.float32)
        factors, sumsq = np.empty(N, dtype=np.float32), np.empty(N, dtype=np.float64)
        rc = self.lib.flm_l2_clip(self.ctx, p_f32(x), N, L, float(clip_norm), p_f32(out), p_f32(factors),
                                  p_f64(sumsq))
        self._check(rc, "flm_l2_clip")
        return (out[0] if one else out), factors, sumsq

    # ------------------------------------- conditional stochastic rounding
    def round_check(self, L: int, frac_bits: int, clip: float, attempts: int = 1):
        """Raise unless round_select can take rows of L parameters at (frac_bits, clip) with `attempts` candidates:
        L > 0, attempts in 1..8, the codec's rule for one client, L ceil(clip 2^frac_bits)^2 <= 2^64 - 1 and
        ceil(L / 16) <= 2^32.  No device call.  flm_round_check."""
        self._check(self.lib.flm_round_check(int(L), int(frac_bits), float(clip), int(attempts)), "flm_round_check")

    def round_bound(self, clip_norm: float, frac_bits: int, d: int, tail: float | None = None, beta: float | None = None) -> int:
        """max_sumsq = Delta^2, the bound on the sum of squares of a rounded row of d coordinates whose float norm the
        L2 clip held to clip_norm (flm_round_bound; Kairouz et al., Algorithm 1).  One of tail = k >= 0 or beta in
        (0, 1], a draw's failure probability, which is turned into k = sqrt(2 ln(1 / beta)) here, in Python: the
        library takes k.  No device call."""
        if (tail is None) == (beta is None):
            raise RuntimeError("round_bound takes exactly one of tail and beta")
        if beta is not None:
            if not 0.0 < float(beta) <= 1.0:
                raise RuntimeError("beta must be in (0, 1]")
            tail = math.sqrt(2.0 * math.log(1.0 / float(beta)))
        out = ctypes.c_uint64(0)
        self._check(self.lib.flm_round_bound(float(clip_norm), int(frac_bits), int(d), float(tail), ctypes.byref(out)),
                    "flm_round_bound")
        return int(out.value)

    def round_select(self, x: np.ndarray, frac_bits: int, clip: float, candidates, max_sumsq: int):
        """For float32 rows x (N, L) or (L,) and candidates (N, A, 32) uint8 (or A 32-byte seeds for one row), A in
        1..8: (dither_seeds (N, 32) uint8, chosen (N,) uint32, sumsq (N, A) uint64).  sumsq[i, a] is the sum of the
        squares of the integers the stochastic encode rounds row i to under candidate a; chosen[i] the first a with
        sumsq <= max_sumsq and dither_seeds[i] that candidate, to be handed to client_encode_*mask as its dither
        seed.  chosen[i] == A: no candidate passed, dither_seeds[i] is candidate 0 and the row must not be sent.
        flm_round_select."""
        x, _ = _float_rows_array(x)
        N, L = x.shape
        if isinstance(candidates, (list, tuple)):
            candidates = _seeds_array(candidates)
        cand = np.ascontiguousarray(candidates, dtype=np.uint8)
        if cand.ndim == 2 and N == 1:
            cand = cand[None]
        if cand.ndim != 3 or cand.shape[0] != N or cand.shape[2] != 32:
            raise RuntimeError("candidates must be (N, A, 32) bytes")
        A = cand.shape[1]
        self.round_check(L, frac_bits, clip, A)
        sumsq = np.empty((N, A), dtype=np.uint64)
        dither = np.empty((N, 32), dtype=np.uint8)
        chosen = np.empty(N, dtype=np.uint32)
        rc = self.lib.flm_round_select(self.ctx, p_f32(x), N, L, int(frac_bits), float(clip), p_u8(cand), A, int(max_sumsq),
                                       p_u64(sumsq), p_u8(dither), p_u32(chosen))
        self._check(rc, "flm_round_select")
        return dither, chosen, sumsq

    def decode_sum(self, total: np.ndarray, frac_bits: int, count: int = 1) -> np.ndarray:
        """float32(int32(total) / (count * 2^frac_bits)): the ring sum as the mean of `count` contributors."""
        total = np.ascontiguousarray(total, dtype=np.uint32)
        if total.ndim != 1:
            raise RuntimeError("total must be a vector")
        out = np.empty(total.shape[0], dtype=np.float32)
        rc = self.lib.flm_decode_sum(self.ctx, p_u32(total), total.shape[0], int(frac_bits), int(count), p_f32(out))
        self._check(rc, "flm_decode_sum")
        return out

    def prg_expand(self, seeds, L: int, slot0: int = 0) -> np.ndarray:
        """PRG(seed_k)[slot0:slot0+L] for every seed; (K, L) uint32."""
        seeds = _seeds_array(seeds)
        out = np.empty((seeds.shape[0], L), dtype=np.uint32)
        rc = self.lib.flm_prg_expand(self.ctx, p_u8(seeds), seeds.shape[0], L, slot0, p_u32(out))
        self._check(rc, "flm_prg_expand")
        return out

    def prg(self, seed: bytes, L: int, slot0: int = 0) -> np.ndarray:
        return self.prg_expand([seed], L, slot0)[0]

    def mask_accumulate(self, seeds, signs, acc: np.ndarray, slot0: int = 0) -> np.ndarray:
        """acc += sum_k signs[k]*PRG(seeds[k])[slot0:] in place; returns acc."""
        if acc.dtype != np.uint32 or not acc.flags.c_contiguous:
            raise RuntimeError("acc must be a C-contiguous uint32 array")
        seeds = _seeds_array(seeds)
        signs = _signs_array(signs, seeds.shape[0])
        rc = self.lib.flm_mask_accumulate(self.ctx, p_u8(seeds), p_i8(signs), seeds.shape[0], p_u32(acc),
                                          acc.shape[0], slot0)
        self._check(rc, "flm_mask_accumulate")
        return acc

    def chacha20_encrypt(self, key: bytes, data: bytes, nonce: bytes = NONCE, counter: int = 0) -> bytes:
        """ChaCha20.new(key=key, nonce=nonce).encrypt(data) (DJB layout), on the GPU."""
        if len(key) != 32 or len(nonce) != 8:
            raise RuntimeError("key must be 32 bytes and nonce 8 bytes")
        n = len(data)
        if n == 0:
            return b""
        src = np.frombuffer(bytes(data), dtype=np.uint8).copy()
        dst = np.empty(n, dtype=np.uint8)
        k = np.frombuffer(bytes(key), dtype=np.uint8).copy()
        nn = np.frombuffer(bytes(nonce), dtype=np.uint8).copy()
        rc = self.lib.flm_chacha20_xor(self.ctx, p_u8(k), p_u8(nn), counter, p_u8(src), p_u8(dst), n)
        self._check(rc, "flm_chacha20_xor")
        return dst.tobytes()

    # ------------------------------------------------------ device tensors
    @staticmethod
    def _stream_handle(stream) -> int:
        """hipStream_t as an int (the c_void_p argtypes take ints as they are)."""
        if stream is None:
            import torch
            return torch.cuda.current_stream().cuda_stream
        if isinstance(stream, int):
            return stream
        return stream.cuda_stream

    def aggregate_unmask_dev(self, rows, seeds, signs, out, L: int | None = None, mask_lo: int = 0,
                             mask_hi: int | None = None, prg_slot0: int = 0, stream=None):
        """Enqueue the device-resident round on `stream` (default: torch's current stream).

        rows: (N, pitch) int32/uint32 CUDA tensor (pitch % 4 == 0, pitch >= L);
        seeds: (K, 32) uint8 CUDA tensor; signs: (K,) int8 CUDA tensor;
        out: CUDA tensor with >= L int32/uint32 elements."""
        # lean checks: this call is the whole host cost of a small round (c2), and every torch
        # attribute read costs ~0.3 us; the other *_dev wrappers check fully (_dev_bytes, _dev_rows)
        N = rows.shape[0] if rows is not None else 0
        width = rows.shape[1] if N else 0
        pitch = rows.stride(0) if N > 1 else width          # a strided row view keeps its true pitch
        if L is None:
            L = width
        if mask_hi is None:
            mask_hi = L
        K = seeds.shape[0] if seeds is not None else 0
        if K and (seeds.shape[-1] != 32 or signs.shape[0] < K):
            raise RuntimeError(f"seeds must be (K, 32) with >= K signs, got {tuple(seeds.shape)}, {tuple(signs.shape)}")
        if (N and width < L) or out.numel() < L:
            raise RuntimeError(f"rows must be (N, >= {L}) and out hold >= {L} elements")
        # plain ints for the c_void_p arguments: this call is the whole host cost of a small
        # round (c2: ~6.5 us of GPU time), so no per-call ctypes wrapper objects
        rc = self.lib.flm_aggregate_unmask_dev(
            self.ctx, rows.data_ptr() if N else 0, pitch, N, seeds.data_ptr() if K else 0,
            signs.data_ptr() if K else 0, K, L, mask_lo, mask_hi, prg_slot0, out.data_ptr(),
            self._stream_handle(stream))
        if rc:
            self._check(rc, "flm_aggregate_unmask_dev")
        return out

    def seed_table_dev(self, seeds, signs, stream=None):
        """Build the device seed schedule (first of the round's two launches)."""
        K = seeds.shape[0] if seeds is not None else 0
        rc = self.lib.flm_seed_table_dev(self.ctx, ctypes.c_void_p(seeds.data_ptr() if K else 0),
                                         ctypes.c_void_p(signs.data_ptr() if K else 0), K,
                                         self._stream_handle(stream))
        self._check(rc, "flm_seed_table_dev")

    def aggregate_dev(self, rows, K: int, out, L: int | None = None, mask_lo: int = 0, mask_hi: int | None = None,
                      prg_slot0: int = 0, stream=None):
        """Row-sum + unmask kernel against the current seed table (second launch)."""
        N = rows.shape[0] if rows is not None else 0
        if L is None:
            L = rows.shape[1] if N else 0
        pitch = _dev_rows(rows, L) if N else 0
        if mask_hi is None:
            mask_hi = L
        _dev_bytes(out, "out", 1, L, 4)
        rc = self.lib.flm_aggregate_dev(self.ctx, ctypes.c_void_p(rows.data_ptr() if N else 0), pitch, N, K, L,
                                        mask_lo, mask_hi, prg_slot0, ctypes.c_void_p(out.data_ptr()),
                                        self._stream_handle(stream))
        self._check(rc, "flm_aggregate_dev")
        return out

    def client_mask_dev(self, seg, seeds_dev, signs, out, L: int, x=None, stream=None):
        """Device client masking: seg/signs host arrays, seeds_dev/x/out CUDA tensors (rows at out.shape[1])."""
        seg, signs, N, K = _client_seeds(seg, signs, seeds_dev)
        if out.dim() != 2 or out.shape[0] < N or out.element_size() != 4 or out.shape[1] < L:
            raise RuntimeError(f"out must be (>= {N}, >= {L}) 32-bit, got {tuple(out.shape)}")
        if x is not None and (tuple(x.shape) != tuple(out.shape) or x.element_size() != 4):
            raise RuntimeError("x must have out's shape and a 32-bit dtype")
        pitch = out.shape[1]
        rc = self.lib.flm_client_mask_dev(self.ctx, ctypes.c_void_p(x.data_ptr() if x is not None else 0), pitch, N,
                                          p_i64(seg), ctypes.c_void_p(seeds_dev.data_ptr()), p_i8(signs), L,
                                          ctypes.c_void_p(out.data_ptr()), self._stream_handle(stream))
        self._check(rc, "flm_client_mask_dev")
        return out

    def _encode_mask_dev(self, fn: str, codec, seg, seeds_dev, signs, out, L: int, x, frac_bits: int, clip: float,
                         pack: int, dither_dev, noise_dev, clipped, stream):
        """The device form of the three encode calls; codec(dither, noise) as in _encode_mask, on device addresses."""
        import torch
        seg, signs, N, K = _client_seeds(seg, signs, seeds_dev)
        Lw = -(-L // pack) if pack > 0 else L
        for name, t, n in (("x", x, L), ("out", out, Lw)):
            if t is None or t.dim() != 2 or t.shape[0] < N or t.shape[1] < n or t.element_size() != 4 or t.stride(1) != 1:
                raise RuntimeError(f"{name} must be (>= {N}, >= {n}) 32-bit with unit column stride")
        if x.dtype != torch.float32:
            raise RuntimeError("x must be float32")
        for name, t in (("dither_dev", dither_dev), ("noise_dev", noise_dev)):
            if t is not None and (tuple(t.shape) != (N, 32) or t.element_size() != 1 or not t.is_contiguous()):
                raise RuntimeError(f"{name} must be a contiguous ({N}, 32) uint8 tensor")
        if clipped is not None and (clipped.dim() != 1 or clipped.shape[0] < N or clipped.element_size() != 4
                                    or not clipped.is_contiguous()):
            raise RuntimeError(f"clipped must be a contiguous (>= {N},) 32-bit tensor")
        ptr = lambda t: ctypes.c_void_p(t.data_ptr() if t is not None else 0)
        rc = getattr(self.lib, fn)(
            self.ctx, ptr(x), x.stride(0) if N > 1 else x.shape[1], N, p_i64(seg), ptr(seeds_dev if K else None), p_i8(signs),
            L, int(frac_bits), float(clip), *codec(ptr(dither_dev), ptr(noise_dev)), ptr(out),
            out.stride(0) if N > 1 else out.shape[1], ptr(clipped), self._stream_handle(stream))
        self._check(rc, fn)
        return out

    def client_encode_mask_dev(self, seg, seeds_dev, signs, out, L: int, x, frac_bits: int, clip: float,
                               dither_dev=None, clipped=None, stream=None):
        """Device client_encode_mask: seg/signs host arrays; seeds_dev (K, 32) uint8, x (>= N, >= L) float32,
        out (>= N, >= L) 32-bit, dither_dev (N, 32) uint8 or None, clipped (>= N,) 32-bit or None: CUDA
        tensors, rows at their own strides.  Enqueued on `stream`; nothing is synchronised."""
        return self._encode_mask_dev("flm_client_encode_mask_dev", lambda d, z: (d,), seg, seeds_dev, signs, out, L, x,
                                     frac_bits, clip, 1, dither_dev, None, clipped, stream)

    def client_encode_pack_mask_dev(self, seg, seeds_dev, signs, out, L: int, x, frac_bits: int, clip: float, pack: int,
                                    dither_dev=None, clipped=None, stream=None):
        """Device client_encode_pack_mask: as client_encode_mask_dev, with x (>= N, >= L) float32 and out
        (>= N, >= ceil(L / pack)) 32-bit.  Enqueued on `stream`; nothing is synchronised."""
        pack = int(pack)
        return self._encode_mask_dev("flm_client_encode_pack_mask_dev", lambda d, z: (pack, d), seg, seeds_dev, signs, out,
                                     L, x, frac_bits, clip, pack, dither_dev, None, clipped, stream)

    def client_encode_noise_mask_dev(self, seg, seeds_dev, signs, out, L: int, x, frac_bits: int, clip: float,
                                     pack: int = 1, dither_dev=None, noise_bits: int = 0, noise_dev=None, clipped=None,
                                     stream=None):
        """Device client_encode_noise_mask: as client_encode_pack_mask_dev (pack 1, 2 or 4), with noise_dev a
        contiguous (N, 32) uint8 tensor of the clients' noise seeds.  Enqueued on `stream`; nothing is synchronised."""
        pack = int(pack)
        return self._encode_mask_dev("flm_client_encode_noise_mask_dev", lambda d, z: (pack, d, int(noise_bits), z), seg,
                                     seeds_dev, signs, out, L, x, frac_bits, clip, pack, dither_dev, noise_dev, clipped,
                                     stream)

    def client_encode_gauss_mask_dev(self, seg, seeds_dev, signs, out, L: int, x, frac_bits: int, clip: float, table_dev,
                                     noise_dev, pack: int = 1, dither_dev=None, clipped=None, stream=None):
        """Device client_encode_gauss_mask: as client_encode_noise_mask_dev, with table_dev a one-dimensional 64-bit
        tensor of 2 * tail entries (8-byte aligned; its contents are not looked at: whatever they are, every field
        stays inside its headroom).  Enqueued on `stream`; nothing is synchronised."""
        pack = int(pack)
        if table_dev is None or table_dev.dim() != 1 or table_dev.element_size() != 8 or table_dev.shape[0] % 2 \
                or table_dev.stride(0) != 1:
            raise RuntimeError("table_dev must be a contiguous tensor of 2 * tail 64-bit entries")
        tail = table_dev.shape[0] // 2
        return self._encode_mask_dev("flm_client_encode_gauss_mask_dev",
                                     lambda d, z: (pack, d, tail, ctypes.c_void_p(table_dev.data_ptr()), z), seg,
                                     seeds_dev, signs, out, L, x, frac_bits, clip, pack, dither_dev, noise_dev, clipped,
                                     stream)

    def decode_sum_dev(self, total, out, L: int, frac_bits: int, count: int = 1, stream=None):
        """out[:L] = decode(total[:L]) on CUDA tensors (32-bit in, float32 out); out may be a float32 view of total."""
        import torch
        if total.element_size() != 4 or total.numel() < L or out.dtype != torch.float32 or out.numel() < L \
                or not total.is_contiguous() or not out.is_contiguous():
            raise RuntimeError(f"total must hold >= {L} 32-bit words and out >= {L} float32, both contiguous")
        rc = self.lib.flm_decode_sum_dev(self.ctx, ctypes.c_void_p(total.data_ptr()), L, int(frac_bits), int(count),
                                         ctypes.c_void_p(out.data_ptr()), self._stream_handle(stream))
        self._check(rc, "flm_decode_sum_dev")
        return out

    def decode_unpack_dev(self, total, out, L: int, frac_bits: int, clip: float, pack: int, count: int = 1, stream=None,
                          noise_bits: int = 0):
        """out[:L] = the packed decode of total[:ceil(L / pack)] on CUDA tensors (32-bit in, float32 out, not views
        of one another).  noise_bits > 0: rows of client_encode_noise_mask.  flm_decode_unpack_noise_dev, which
        without noise is flm_decode_unpack_dev."""
        import torch
        pack = int(pack)
        Lw = -(-L // pack) if pack > 0 else L
        if total.element_size() != 4 or total.numel() < Lw or out.dtype != torch.float32 or out.numel() < L \
                or not total.is_contiguous() or not out.is_contiguous():
            raise RuntimeError(f"total must hold >= {Lw} 32-bit words and out >= {L} float32, both contiguous")
        rc = self.lib.flm_decode_unpack_noise_dev(self.ctx, ctypes.c_void_p(total.data_ptr()), L, int(frac_bits), float(clip),
                                                  pack, int(noise_bits), int(count), ctypes.c_void_p(out.data_ptr()),
                                                  self._stream_handle(stream))
        self._check(rc, "flm_decode_unpack_noise_dev")
        return out

    def decode_unpack_mod_dev(self, total, out, L: int, frac_bits: int, clip: float, pack: int, count: int = 1, stream=None,
                              noise_bits: int = 0, guard: int = 1, stats=None):
        """decode_unpack_dev of a sum taken modulo the field (decode_unpack_mod) on CUDA tensors; out may not overlap
        total.  stats: a contiguous CUDA tensor of >= 2 32-bit words, zeroed on the stream and then holding (near,
        max_abs), or None.  Enqueued on `stream`; nothing is synchronised.  Returns (out, stats).
        flm_decode_unpack_mod_dev."""
        import torch
        pack = int(pack)
        Lw = -(-L // pack) if pack > 0 else L
        if total.element_size() != 4 or total.numel() < Lw or out.dtype != torch.float32 or out.numel() < L \
                or not total.is_contiguous() or not out.is_contiguous():
            raise RuntimeError(f"total must hold >= {Lw} 32-bit words and out >= {L} float32, both contiguous")
        if stats is not None and (stats.element_size() != 4 or stats.numel() < 2 or not stats.is_contiguous()):
            raise RuntimeError("stats must hold >= 2 32-bit words, contiguous")
        rc = self.lib.flm_decode_unpack_mod_dev(self.ctx, ctypes.c_void_p(total.data_ptr()), L, int(frac_bits), float(clip),
                                                pack, int(noise_bits), int(count), int(guard),
                                                ctypes.c_void_p(out.data_ptr()),
                                                ctypes.c_void_p(stats.data_ptr()) if stats is not None else None,
                                                self._stream_handle(stream))
        self._check(rc, "flm_decode_unpack_mod_dev")
        return out, stats

    def rotate_dev(self, x, out, L: int, log2_block: int, sign_bits, inverse: bool = False, nonfinite=None, stream=None):
        """Device rotate: x and out (>= N, >= row length) float32 CUDA tensors with unit column stride, rows at their
        own strides (out may be x); forward reads L and writes L_rot floats a row, inverse reads L_rot and writes L.
        sign_bits: >= ceil(L_rot / 32) 32-bit words, prg_expand_dev of the key (K = 1); nonfinite (>= N,) 32-bit or
        None, forward only.  Enqueued on `stream`; nothing is synchronised.  flm_rotate_dev."""
        L_rot = self.rotate_check(L, log2_block)
        N = x.shape[0] if x.dim() == 2 else -1
        xp = self._float_rows("x", x, N, L_rot if inverse else L)
        op = self._float_rows("out", out, N, L if inverse else L_rot)
        _dev_vector("sign_bits", sign_bits, -(-L_rot // 32), 4, "32-bit", flat=True)
        _dev_vector("nonfinite", nonfinite, N, 4, "32-bit")
        rc = self.lib.flm_rotate_dev(self.ctx, _vp(x), xp, N, int(L), int(log2_block), _vp(sign_bits), int(bool(inverse)),
                                     _vp(out), op, _vp(nonfinite), self._stream_handle(stream))
        self._check(rc, "flm_rotate_dev")
        return out

    @staticmethod
    def _float_rows(name: str, t, N: int, n: int) -> int:
        """The row pitch of a (N, >= n) float32 CUDA tensor with unit column stride."""
        import torch
        if t.dim() != 2 or t.shape[0] != N or t.shape[1] < n or t.dtype != torch.float32 or t.stride(1) != 1:
            raise RuntimeError(f"{name} must be ({N}, >= {n}) float32 with unit column stride")
        return t.stride(0) if N > 1 else t.shape[1]

    def l2_factors_dev(self, x, L: int, clip_norm: float, work, factors, sumsq=None, stream=None):
        """Device L2 factors: x (N, >= L) float32 rows at their own stride; work >= l2_clip_check(L, clip_norm, N)
        float64, the caller's, one per stream in flight; factors (>= N,) float32 and sumsq (>= N,) float64 or None are
        written.  Two launches enqueued on `stream`; nothing is synchronised.  flm_l2_factors_dev."""
        import torch
        N = x.shape[0] if x.dim() == 2 else -1
        need = self.l2_clip_check(L, clip_norm, N)
        pitch = self._float_rows("x", x, N, L)
        for name, t, n, dt in (("work", work, need, torch.float64), ("factors", factors, N, torch.float32),
                               ("sumsq", sumsq, N, torch.float64)):
            _dev_vector(name, t, n, dt)
        rc = self.lib.flm_l2_factors_dev(self.ctx, _vp(x), pitch, N, int(L), float(clip_norm), _vp(work), _vp(factors),
                                         _vp(sumsq), self._stream_handle(stream))
        self._check(rc, "flm_l2_factors_dev")
        return factors

    def scale_rows_dev(self, x, out, L: int, factors, stream=None):
        """Device scale: out[row, :L] = x[row, :L] factors[row], float32 rows at their own strides (out may be x);
        nothing behind L is written.  Enqueued on `stream`; nothing is synchronised.  flm_scale_rows_dev."""
        import torch
        N = x.shape[0] if x.dim() == 2 else -1
        xp, op = self._float_rows("x", x, N, L), self._float_rows("out", out, N, L)
        _dev_vector("factors", factors, N, torch.float32, "float32")
        rc = self.lib.flm_scale_rows_dev(self.ctx, _vp(x), xp, N, int(L), _vp(factors), _vp(out), op,
                                         self._stream_handle(stream))
        self._check(rc, "flm_scale_rows_dev")
        return out

    def rotate_clip_dev(self, x, out, L: int, log2_block: int, sign_bits, factors, nonfinite=None, stream=None):
        """rotate_dev's forward direction with the L2 clip's multiply by factors[row] (l2_factors_dev) in its load:
        scale_rows_dev followed by rotate_dev, bit for bit, in one pass.  flm_rotate_clip_dev."""
        import torch
        L_rot = self.rotate_check(L, log2_block)
        N = x.shape[0] if x.dim() == 2 else -1
        xp, op = self._float_rows("x", x, N, L), self._float_rows("out", out, N, L_rot)
        _dev_vector("sign_bits", sign_bits, -(-L_rot // 32), 4, "32-bit", flat=True)
        _dev_vector("factors", factors, N, torch.float32, "float32")
        _dev_vector("nonfinite", nonfinite, N, 4, "32-bit")
        rc = self.lib.flm_rotate_clip_dev(self.ctx, _vp(x), xp, N, int(L), int(log2_block), _vp(sign_bits), _vp(factors),
                                          _vp(out), op, _vp(nonfinite), self._stream_handle(stream))
        self._check(rc, "flm_rotate_clip_dev")
        return out

    def round_select_dev(self, x, L: int, frac_bits: int, clip: float, candidates, max_sumsq: int, sumsq, dither, chosen,
                         stream=None):
        """Device round_select: x (N, >= L) float32 rows at their own stride; candidates a contiguous (N, A, 32) uint8
        tensor; sumsq >= N A 64-bit words, dither a contiguous (N, 32) uint8 tensor and chosen (>= N,) 32-bit are
        written.  Two launches enqueued on `stream`; nothing is synchronised, and dither may go straight into
        client_encode_*mask_dev on the same stream.  flm_round_select_dev."""
        N = x.shape[0] if x.dim() == 2 else -1
        pitch = self._float_rows("x", x, N, L)
        if candidates.dim() != 3 or candidates.shape[0] != N or candidates.shape[2] != 32 or candidates.element_size() != 1 \
                or not candidates.is_contiguous():
            raise RuntimeError(f"candidates must be a contiguous ({N}, A, 32) uint8 tensor")
        A = candidates.shape[1]
        self.round_check(L, frac_bits, clip, A)
        _dev_vector("sumsq", sumsq, N * A, 8, "64-bit", flat=True)
        _dev_bytes(dither, "dither", 32, N)
        _dev_vector("chosen", chosen, N, 4, "32-bit")
        rc = self.lib.flm_round_select_dev(self.ctx, _vp(x), pitch, N, int(L), int(frac_bits), float(clip), _vp(candidates), A,
                                           int(max_sumsq), _vp(sumsq), _vp(dither), _vp(chosen), self._stream_handle(stream))
        self._check(rc, "flm_round_select_dev")
        return dither

    def prg_expand_dev(self, seeds_dev, out, L: int, slot0: int = 0, stream=None):
        K = seeds_dev.shape[0]
        rc = self.lib.flm_prg_expand_dev(self.ctx, ctypes.c_void_p(seeds_dev.data_ptr()), K, L, slot0,
                                         ctypes.c_void_p(out.data_ptr()), out.shape[1], self._stream_handle(stream))
        self._check(rc, "flm_prg_expand_dev")
        return out

    # ------------------------------------------------------------ P-256
    def ec_mul_wire(self, points_w: np.ndarray, scalars_w: np.ndarray):
        """Batched k_i * P_i on wire arrays: points (n, 64) and scalars (n, 32) uint8 big endian.
        Returns (out (n, 64) uint8, flags (n,) uint32; bit 2 = infinity, returned as zeros)."""
        pw = np.ascontiguousarray(points_w, np.uint8).reshape(-1, 64)
        sw = np.ascontiguousarray(scalars_w, np.uint8).reshape(-1, 32)
        n = pw.shape[0]
        if sw.shape[0] != n:
            raise RuntimeError(f"{sw.shape[0]} scalars for {n} points")
        out = np.zeros((n, 64), np.uint8)
        fl = np.zeros(n, np.uint32)
        if n:
            self._check(self.lib.flm_ec_mul(self.ctx, p_u8(pw), p_u8(sw), n, p_u8(out), p_u32(fl)), "flm_ec_mul")
        return out, fl

    def hash_to_curve_wire(self, msgs):
        """ecchash.hash_str_to_curve(msg, 2, n, 1, 48, XMD SHA-256) of each message (str or bytes,
        <= 64 bytes) on the GPU (flm_hash_to_curve).  Returns (out (n, 64) uint8 wire x||y,
        flags (n,) uint32; bit 2 = infinity)."""
        raw = [m.encode() if isinstance(m, str) else bytes(m) for m in msgs]
        n = len(raw)
        buf = np.zeros((max(n, 1), 64), np.uint8)
        lens = np.zeros(max(n, 1), np.uint32)
        for i, m in enumerate(raw):
            if len(m) > 64:
                raise RuntimeError(f"message {i} is {len(m)} bytes (at most 64)")
            buf[i, :len(m)] = np.frombuffer(m, np.uint8)
            lens[i] = len(m)
        out = np.zeros((n, 64), np.uint8)
        fl = np.zeros(n, np.uint32)
        if n:
            self._check(self.lib.flm_hash_to_curve(self.ctx, p_u8(buf), p_u32(lens), n, p_u8(out), p_u32(fl)),
                        "flm_hash_to_curve")
        return out, fl

    def hash_to_curve_decimal(self, v0: int = 0, n: int = 1 << 16):
        """hash_str_to_curve(str(v)) for v in [v0, v0 + n) in one launch (flm_hash_to_curve_decimal):
        with the defaults, every h_ijt a client can hash (SA_ClientAgent.py:280).  (out, flags) as
        hash_to_curve_wire."""
        out = np.zeros((n, 64), np.uint8)
        fl = np.zeros(n, np.uint32)
        if n:
            self._check(self.lib.flm_hash_to_curve_decimal(self.ctx, int(v0), int(n), p_u8(out), p_u32(fl)),
                        "flm_hash_to_curve_decimal")
        return out, fl

    def hash_to_curve_decimal_dev(self, v0: int, n: int, out, flags, stream=None):
        """Device form: out (n, 64) uint8 and flags (n,) int32/uint32 CUDA tensors; enqueued on `stream`."""
        _dev_bytes(out, "out", 64, n)
        _dev_bytes(flags, "flags", 1, n, 4)
        self._check(self.lib.flm_hash_to_curve_decimal_dev(self.ctx, int(v0), int(n), out.data_ptr(), flags.data_ptr(),
                                                           self._stream_handle(stream)),
                    "flm_hash_to_curve_decimal_dev")
        return out, flags

    def ec_mul(self, points, scalars) -> list:
        """[k_i * P_i] for affine points (x, y) and integer scalars (flm_ec_mul).

        The ECDH / ElGamal / decryption-share products of SA_ClientAgent.py:256-263,
        :434-447 and :397-400, batched.  Infinity comes back as None."""
        from .crypto import points_from_wire, points_to_wire, scalars_to_wire
        if len(scalars) != len(points):
            raise RuntimeError(f"{len(scalars)} scalars for {len(points)} points")
        if not points:
            return []
        out, fl = self.ec_mul_wire(points_to_wire(points), scalars_to_wire(scalars))
        return points_from_wire(out, fl)

    def ec_combine_wire(self, c1_w, shares_w, lambdas_w, negate: bool = True):
        """flm_ec_combine on wire arrays: c1 (D, 64) or None, shares (T, D, 64), lambdas (T, 32).
        Returns (points (D, 64), seeds (D, 32), flags (D,))."""
        sh = np.ascontiguousarray(shares_w, np.uint8)
        T = sh.shape[0]
        lw = np.ascontiguousarray(lambdas_w, np.uint8).reshape(-1, 32)
        if lw.shape[0] != T:
            raise RuntimeError(f"{lw.shape[0]} coefficients for {T} share sets")
        D = c1_w.shape[0] if c1_w is not None else (sh.shape[1] if T else 0)
        if T and (sh.ndim != 3 or sh.shape[1] != D or sh.shape[2] != 64):
            raise RuntimeError("shares must be (T, D, 64)")
        pts = np.zeros((D, 64), np.uint8)
        seeds = np.zeros((D, 32), np.uint8)
        fl = np.zeros(D, np.uint32)
        if D == 0:
            return pts, seeds, fl
        cw = np.ascontiguousarray(c1_w, np.uint8) if c1_w is not None else None
        if not T:
            sh, lw = np.zeros((1, 64), np.uint8), np.zeros((1, 32), np.uint8)
        rc = self.lib.flm_ec_combine(self.ctx, p_u8(cw) if cw is not None else None, p_u8(sh), p_u8(lw), T, D,
                                     1 if negate else 0, p_u8(pts), p_u8(seeds), p_u32(fl))
        self._check(rc, "flm_ec_combine")
        return pts, seeds, fl

    def ec_combine(self, c1, shares_by_term, lambdas, negate: bool = True):
        """Threshold-ElGamal combine + seed derivation (SA_ServiceAgent.py:542-585).

        c1: D affine points (or None: base = infinity); shares_by_term: T lists of D
        points (share_{j,i} = sk_j * c0_i); lambdas: T Lagrange coefficients.
        Returns (points, seeds): point_i = c1_i - sum_j lambda_j share_{j,i}
        (+ when negate is False) and seed_i = SHA-256(x||y) as 32 bytes."""
        from .crypto import points_from_wire, points_to_wire, scalars_to_wire
        T = len(lambdas)
        D = len(c1) if c1 is not None else (len(shares_by_term[0]) if T else 0)
        if len(shares_by_term) != T or any(len(s) != D for s in shares_by_term):
            raise RuntimeError("shares must be T lists of D points")
        if D == 0:
            return [], []
        sh = np.stack([points_to_wire(s) for s in shares_by_term]) if T else np.zeros((0, D, 64), np.uint8)
        lw = scalars_to_wire(lambdas) if T else np.zeros((0, 32), np.uint8)
        pts, seeds, fl = self.ec_combine_wire(points_to_wire(c1) if c1 is not None else None, sh, lw, negate)
        return points_from_wire(pts, fl), [bytes(r) for r in seeds]

    def shamir_combine(self, shares_by_term, lambdas) -> list:
        """m_i = sum_j lambda_j y_{j,i} mod n as 32-byte big-endian seeds (SA_ServiceAgent.py:506-526).
        shares_by_term: T sequences of M integers (< 2^256); lambdas: T integers (< n)."""
        from .crypto import scalars_to_wire
        T = len(lambdas)
        if len(shares_by_term) != T:
            raise RuntimeError(f"{len(shares_by_term)} share lists for {T} coefficients")
        M = len(shares_by_term[0]) if T else 0
        if any(len(s) != M for s in shares_by_term):
            raise RuntimeError("share lists differ in length")
        if M == 0:
            return []
        sh = np.stack([scalars_to_wire(s) for s in shares_by_term])
        out = np.zeros((M, 32), np.uint8)
        rc = self.lib.flm_shamir_combine(self.ctx, p_u8(sh), p_u8(scalars_to_wire(lambdas)), T, M, p_u8(out))
        self._check(rc, "flm_shamir_combine")
        return [bytes(r) for r in out]

    def shamir_combine_dev(self, shares, lambdas, seeds_out, stream=None):
        """Device form: shares (T, M, 32), lambdas (T, 32) uint8 CUDA tensors -> seeds_out (M, 32)."""
        _need(shares.dim() == 3, "shares must be (T, M, 32)")
        T, M = shares.shape[0], shares.shape[1]
        _dev_bytes(shares, "shares", 32, T * M)
        _dev_bytes(lambdas, "lambdas", 32, T)
        _dev_bytes(seeds_out, "seeds_out", 32, M)
        rc = self.lib.flm_shamir_combine_dev(self.ctx, ctypes.c_void_p(shares.data_ptr()),
                                             ctypes.c_void_p(lambdas.data_ptr()), T, M,
                                             ctypes.c_void_p(seeds_out.data_ptr()), self._stream_handle(stream))
        self._check(rc, "flm_shamir_combine_dev")
        return seeds_out

    def shamir_deal_wire(self, coeffs_w, xs) -> np.ndarray:
        """flm_shamir_deal on wire arrays: coeffs (T, M, 32) uint8 big endian (term 0 the secrets, any
        value < 2^256), xs C non-zero points -> shares (C, M, 32) uint8, each < n; row c is ready to
        be a shares[j] of shamir_combine.  No Python big ints on the way."""
        cw = np.ascontiguousarray(coeffs_w, np.uint8)
        if cw.ndim != 3 or cw.shape[2] != 32:
            raise RuntimeError("coeffs must be (T, M, 32)")
        T, M = cw.shape[0], cw.shape[1]
        x = np.asarray(xs)
        if x.ndim != 1 or (x.size and (x.dtype.kind not in "ui" or x.min() < 0 or x.max() > 0xFFFFFFFF)):
            raise RuntimeError("xs must be a 1-D sequence of integers below 2^32")
        x = np.ascontiguousarray(x, np.uint32)
        out = np.zeros((x.shape[0], M, 32), np.uint8)
        rc = self.lib.flm_shamir_deal(self.ctx, p_u8(cw), T, M, p_u32(x), x.shape[0], p_u8(out))
        self._check(rc, "flm_shamir_deal")
        return out

    def shamir_deal(self, coeffs_by_term, xs) -> list:
        """y[c][i] = sum_j coeffs_by_term[j][i] * xs[c]^j mod n (SA_ClientAgent.py:218-220, the
        inverse of shamir_combine).  coeffs_by_term: T sequences of M integers (< 2^256), term 0 the
        secrets; xs: C non-zero integers (< 2^32).  Returns C lists of M integers."""
        from .crypto import scalars_to_wire
        T = len(coeffs_by_term)
        M = len(coeffs_by_term[0]) if T else 0
        if any(len(c) != M for c in coeffs_by_term):
            raise RuntimeError("coefficient lists differ in length")
        if any(not 0 <= int(v) < (1 << 256) for c in coeffs_by_term for v in c):
            raise RuntimeError("coefficients must be in [0, 2^256)")
        if any(not 0 <= int(v) < (1 << 32) for v in xs):
            raise RuntimeError("xs must be in [1, 2^32)")
        cw = (np.stack([scalars_to_wire(c) for c in coeffs_by_term]) if T and M
              else np.zeros((T, M, 32), np.uint8))
        out = self.shamir_deal_wire(cw, np.array([int(v) for v in xs], np.uint32))
        return [[int.from_bytes(bytes(r), "big") for r in row] for row in out]

    def shamir_deal_dev(self, coeffs, xs, shares_out, stream=None):
        """Device form: coeffs (T, M, 32) uint8, xs (C,) int32 (non-zero; read as uint32) CUDA tensors
        -> shares_out (C, M, 32) uint8, enqueued on `stream`."""
        _need(coeffs.dim() == 3, "coeffs must be (T, M, 32)")
        T, M = coeffs.shape[0], coeffs.shape[1]
        C = xs.numel() if xs is not None else 0
        _dev_bytes(coeffs, "coeffs", 32, T * M)
        _dev_bytes(xs, "xs", 1, C, 4)
        _dev_bytes(shares_out, "shares_out", 32, C * M)
        rc = self.lib.flm_shamir_deal_dev(self.ctx, ctypes.c_void_p(coeffs.data_ptr()), T, M,
                                          ctypes.c_void_p(xs.data_ptr()), C,
                                          ctypes.c_void_p(shares_out.data_ptr()), self._stream_handle(stream))
        self._check(rc, "flm_shamir_deal_dev")
        return shares_out

    def aes_gcm_xor_wire(self, keys, nonces, data) -> np.ndarray:
        """AES.new(key, AES.MODE_GCM, nonce=nonce).encrypt(data) with the tag dropped, for n messages
        (flm_aes_gcm_xor; SA_ClientAgent.py:227-244, and the decryption of :402-420 -- the same XOR).
        keys (n, 16), nonces (n, 12 or 16), data (n, len) uint8 with 1 <= len <= 256 -> (n, len)."""
        k, nc, _, d = self._gcm_rows(keys, nonces, None, data)
        n = k.shape[0]
        out = np.zeros_like(d)
        rc = self.lib.flm_aes_gcm_xor(self.ctx, p_u8(k), p_u8(nc), nc.shape[1], p_u8(d), p_u8(out), d.shape[1], n)
        self._check(rc, "flm_aes_gcm_xor")
        return out

    def aes_gcm_xor_dev(self, keys, nonces, data, out=None, stream=None):
        """Device form: keys (n, 16), nonces (n, 12 or 16), data (n, len) uint8 CUDA tensors -> out
        (n, len), which may be `data` itself (the default: in place); enqueued on `stream`."""
        _need(keys.dim() == 2 and nonces.dim() == 2 and data.dim() == 2,
              "keys must be (n, 16), nonces (n, nonce_len), data (n, len)")
        out = data if out is None else out
        n, ln = data.shape
        _dev_bytes(keys, "keys", 16, n)
        _dev_bytes(nonces, "nonces", nonces.shape[1], n)
        _dev_bytes(data, "data", ln, n)
        _dev_bytes(out, "out", ln, n)
        _need(keys.shape[0] == n and nonces.shape[0] == n, f"{keys.shape[0]} keys and {nonces.shape[0]} nonces "
              f"for {n} messages")
        rc = self.lib.flm_aes_gcm_xor_dev(self.ctx, _vp(keys), _vp(nonces), nonces.shape[1], _vp(data), _vp(out), ln, n,
                                          self._stream_handle(stream))
        self._check(rc, "flm_aes_gcm_xor_dev")
        return out

    @staticmethod
    def _gcm_rows(keys, nonces, aad, data):
        """The host arrays of aes_gcm_seal_wire / aes_gcm_open_wire: (keys, nonces, aad or None, data)."""
        k = np.ascontiguousarray(keys, np.uint8)
        nc = np.ascontiguousarray(nonces, np.uint8)
        d = np.ascontiguousarray(data, np.uint8)
        if k.ndim != 2 or k.shape[1] != 16 or nc.ndim != 2 or d.ndim != 2:
            raise RuntimeError("keys must be (n, 16), nonces (n, nonce_len), data (n, len)")
        n = k.shape[0]
        if nc.shape[0] != n or d.shape[0] != n:
            raise RuntimeError(f"{n} keys for {nc.shape[0]} nonces and {d.shape[0]} messages")
        a = None
        if aad is not None:
            a = np.ascontiguousarray(aad, np.uint8)
            if a.ndim != 2 or a.shape[0] != n:
                raise RuntimeError(f"aad must be ({n}, aad_len)")
            if a.shape[1] == 0:
                a = None
        return k, nc, a, d

    def aes_gcm_seal_wire(self, keys, nonces, data, aad=None):
        """AES-128-GCM with its tag for n messages (flm_aes_gcm_seal): what pycryptodome's
        update(aad) + encrypt_and_digest(data) returns.  keys (n, 16), nonces (n, 12 or 16), data
        (n, len) with 0 <= len <= 256, aad (n, aad_len <= 64) or None -> (ct (n, len), tags (n, 16))."""
        k, nc, a, d = self._gcm_rows(keys, nonces, aad, data)
        n = k.shape[0]
        out = np.zeros_like(d)
        tags = np.zeros((n, 16), np.uint8)
        rc = self.lib.flm_aes_gcm_seal(self.ctx, p_u8(k), p_u8(nc), nc.shape[1], p_u8(a) if a is not None else None,
                                       a.shape[1] if a is not None else 0, p_u8(d), p_u8(out), d.shape[1], p_u8(tags), n)
        self._check(rc, "flm_aes_gcm_seal")
        return out, tags

    def aes_gcm_open_wire(self, keys, nonces, data, tags, aad=None):
        """The verifying inverse (flm_aes_gcm_open): -> (plain (n, len), ok (n,) bool).  A row whose tag
        does not verify has ok False and len zero bytes, never unauthenticated plaintext."""
        k, nc, a, d = self._gcm_rows(keys, nonces, aad, data)
        n = k.shape[0]
        t = np.ascontiguousarray(tags, np.uint8)
        if t.shape != (n, 16):
            raise RuntimeError(f"tags must be ({n}, 16)")
        out = np.zeros_like(d)
        ok = np.zeros(n, np.uint8)
        rc = self.lib.flm_aes_gcm_open(self.ctx, p_u8(k), p_u8(nc), nc.shape[1], p_u8(a) if a is not None else None,
                                       a.shape[1] if a is not None else 0, p_u8(d), p_u8(t), p_u8(out), d.shape[1],
                                       p_u8(ok), n)
        self._check(rc, "flm_aes_gcm_open")
        return out, ok.astype(bool)

    def _gcm_dev_args(self, keys, nonces, aad, data, out, tags):
        _need(keys.dim() == 2 and nonces.dim() == 2 and data.dim() == 2,
              "keys must be (n, 16), nonces (n, nonce_len), data (n, len)")
        n, ln = data.shape
        _need(keys.shape[0] == n and nonces.shape[0] == n, f"{keys.shape[0]} keys and {nonces.shape[0]} nonces "
              f"for {n} messages")
        _dev_bytes(keys, "keys", 16, n)
        _dev_bytes(nonces, "nonces", nonces.shape[1], n)
        _dev_bytes(data, "data", ln, n)
        _dev_bytes(out, "out", ln, n)
        _dev_bytes(tags, "tags", 16, n)
        al = 0
        if aad is not None and aad.dim() == 2 and aad.shape[1] > 0:
            al = aad.shape[1]
            _dev_bytes(aad, "aad", al, n)
        else:
            aad = None
        return n, ln, aad, al

    def aes_gcm_seal_dev(self, keys, nonces, data, tags_out, out=None, aad=None, stream=None):
        """Device form of aes_gcm_seal_wire: uint8 CUDA tensors, tags_out (n, 16); out (n, len) may be
        `data` itself (the default: in place); enqueued on `stream`, nothing staged or awaited."""
        out = data if out is None else out
        n, ln, aad, al = self._gcm_dev_args(keys, nonces, aad, data, out, tags_out)
        rc = self.lib.flm_aes_gcm_seal_dev(self.ctx, _vp(keys), _vp(nonces), nonces.shape[1], _vp(aad), al, _vp(data),
                                           _vp(out), ln, _vp(tags_out), n, self._stream_handle(stream))
        self._check(rc, "flm_aes_gcm_seal_dev")
        return out, tags_out

    def aes_gcm_open_dev(self, keys, nonces, data, tags, ok_out, out=None, aad=None, stream=None):
        """Device form of aes_gcm_open_wire: ok_out (n,) uint8; out may be `data` itself (the default)."""
        out = data if out is None else out
        n, ln, aad, al = self._gcm_dev_args(keys, nonces, aad, data, out, tags)
        _dev_bytes(ok_out, "ok_out", 1, n)
        rc = self.lib.flm_aes_gcm_open_dev(self.ctx, _vp(keys), _vp(nonces), nonces.shape[1], _vp(aad), al, _vp(data),
                                           _vp(tags), _vp(out), ln, _vp(ok_out), n, self._stream_handle(stream))
        self._check(rc, "flm_aes_gcm_open_dev")
        return out, ok_out

    def ecdsa_verify_wire(self, pk_w, digests_w, sigs_w):
        """flm_ecdsa_verify on wire arrays: public keys (n, 64) x||y, digests (n, 32), signatures (n, 64)
        r||s, uint8 big endian -> (ok (n,) bool, flags (n,) uint32).  The verdict of FIPS 186-4 /
        OpenSSL's ECDSA_do_verify; flags bit 0: r or s outside [1, n-1], bit 1: key not a valid point
        (64 zero bytes included), bit 2: u1 G + u2 Q at infinity.  An invalid row is a result, not an
        error (the committee's check the reference leaves out, SA_ClientAgent.py:387)."""
        pk = np.ascontiguousarray(pk_w, np.uint8)
        dg = np.ascontiguousarray(digests_w, np.uint8)
        sg = np.ascontiguousarray(sigs_w, np.uint8)
        if pk.ndim != 2 or pk.shape[1] != 64 or dg.ndim != 2 or dg.shape[1] != 32 or sg.ndim != 2 or sg.shape[1] != 64:
            raise RuntimeError("public keys must be (n, 64), digests (n, 32), signatures (n, 64)")
        n = pk.shape[0]
        if dg.shape[0] != n or sg.shape[0] != n:
            raise RuntimeError(f"{n} keys for {dg.shape[0]} digests and {sg.shape[0]} signatures")
        ok = np.zeros(n, np.uint8)
        fl = np.zeros(n, np.uint32)
        rc = self.lib.flm_ecdsa_verify(self.ctx, p_u8(pk), p_u8(dg), p_u8(sg), n, p_u8(ok), p_u32(fl))
        self._check(rc, "flm_ecdsa_verify")
        return ok.astype(bool), fl

    def ecdsa_verify(self, pubs, msgs, sigs) -> list:
        """ECDSA-SHA256 verification of n (public key, message, 64-byte r||s signature) rows in one
        launch: what crypto.ecdsa_verify answers row by row.  pubs: affine (x, y) integer pairs; None
        (infinity), coordinates outside [0, 2^256) and signatures of another length are invalid."""
        import hashlib
        n = len(pubs)
        if len(msgs) != n or len(sigs) != n:
            raise RuntimeError(f"{n} keys for {len(msgs)} messages and {len(sigs)} signatures")
        pk = np.zeros((n, 64), np.uint8)
        dg = np.zeros((n, 32), np.uint8)
        sg = np.zeros((n, 64), np.uint8)
        for i, (pub, msg, sig) in enumerate(zip(pubs, msgs, sigs)):
            if pub is None or len(sig) != 64 or not all(0 <= int(c) < (1 << 256) for c in pub):
                continue    # the row stays zero: key 0^64 and r = s = 0 are both refused
            pk[i] = np.frombuffer(int(pub[0]).to_bytes(32, "big") + int(pub[1]).to_bytes(32, "big"), np.uint8)
            dg[i] = np.frombuffer(hashlib.sha256(bytes(msg)).digest(), np.uint8)
            sg[i] = np.frombuffer(bytes(sig), np.uint8)
        ok, _ = self.ecdsa_verify_wire(pk, dg, sg)
        return [bool(v) for v in ok]

    def ecdsa_verify_dev(self, pubkeys, digests, sigs, ok_out, flags=None, stream=None):
        """Device form: pubkeys (n, 64), digests (n, 32), sigs (n, 64) uint8 CUDA tensors -> ok_out (n,)
        uint8 and, unless None, flags (n,) int32, enqueued on `stream` (nothing staged or awaited)."""
        _need(pubkeys.dim() == 2, "pubkeys must be (n, 64)")
        n = pubkeys.shape[0]
        _dev_bytes(pubkeys, "pubkeys", 64, n)
        _dev_bytes(digests, "digests", 32, n)
        _dev_bytes(sigs, "sigs", 64, n)
        _dev_bytes(ok_out, "ok_out", 1, n)
        if flags is not None:
            _dev_bytes(flags, "flags", 1, n, 4)
        rc = self.lib.flm_ecdsa_verify_dev(self.ctx, _vp(pubkeys), _vp(digests), _vp(sigs), n, _vp(ok_out), _vp(flags),
                                           self._stream_handle(stream))
        self._check(rc, "flm_ecdsa_verify_dev")
        return ok_out

    def feldman_verify_wire(self, commitments_w, dealer, xs, shares_w, x_bits=None, points=False):
        """flm_feldman_verify on wire arrays: commitments (T, M, 64) term-major wire points (64 zero bytes:
        infinity, a valid term), dealer (n,) indices < M or None (row i: dealer i % M), xs (n,) uint32,
        shares (n, 32) big endian -> (ok (n,) bool, flags (n,) uint32, points (n, 64) or None).
        ok[i]: shares[i] G == sum_k xs[i]^k C[k][dealer[i]] (agent/dkg/SA_ClientAgent.py:219-228).
        x_bits None: the bit length of max(xs), at least 1.  flags bit 0: share >= n, bit 1: a
        commitment off the curve, bit 2: the right-hand side at infinity, bit 3: x >= 2^x_bits.  A
        failed check is a result, not an error."""
        cw = np.ascontiguousarray(commitments_w, np.uint8)
        sw = np.ascontiguousarray(shares_w, np.uint8)
        xv = np.ascontiguousarray(xs, np.uint32).reshape(-1)
        if cw.ndim != 3 or cw.shape[2] != 64 or sw.ndim != 2 or sw.shape[1] != 32:
            raise RuntimeError("commitments must be (T, M, 64), shares (n, 32)")
        T, M, n = cw.shape[0], cw.shape[1], sw.shape[0]
        if xv.shape[0] != n:
            raise RuntimeError(f"{n} shares for {xv.shape[0]} evaluation points")
        dv = None
        if dealer is not None:
            dv = np.ascontiguousarray(dealer, np.uint32).reshape(-1)
            if dv.shape[0] != n:
                raise RuntimeError(f"{n} shares for {dv.shape[0]} dealer indices")
        if x_bits is None:
            x_bits = max(1, int(xv.max()).bit_length()) if n else 1
        ok = np.zeros(n, np.uint8)
        fl = np.zeros(n, np.uint32)
        pts = np.zeros((n, 64), np.uint8) if points else None
        rc = self.lib.flm_feldman_verify(self.ctx, p_u8(cw), T, M, p_u32(dv) if dv is not None else None, p_u32(xv),
                                         int(x_bits), p_u8(sw), n, p_u8(ok), p_u8(pts) if points else None, p_u32(fl))
        self._check(rc, "flm_feldman_verify")
        return ok.astype(bool), fl, pts

    def feldman_verify(self, commitments, dealer, xs, shares, x_bits=None, points=False):
        """Feldman share checks for n (dealer, x, share) rows in one launch: what crypto.feldman_verify
        answers row by row.  commitments[k][d]: term k of dealer d, an affine (x, y) integer pair or
        None (infinity); dealer: n indices or None (row i: dealer i % M); shares: integers (one outside
        [0, 2^256) is refused like any share >= n).  -> the verdicts, a list of bool; with points=True
        (verdicts, [F_d(x) as (x, y) or None])."""
        from .crypto import points_from_wire, points_to_wire
        T = len(commitments)
        M = len(commitments[0]) if T else 0
        cw = (np.stack([points_to_wire(row) for row in commitments]) if T and M else np.zeros((T, M, 64), np.uint8))
        n = len(shares)
        sw = np.full((n, 32), 0xFF, np.uint8)   # 2^256 - 1 >= n: refused
        for i, s in enumerate(shares):
            if 0 <= int(s) < (1 << 256):
                sw[i] = np.frombuffer(int(s).to_bytes(32, "big"), np.uint8)
        ok, fl, pts = self.feldman_verify_wire(cw, dealer, [int(v) for v in xs], sw, x_bits, points)
        verdicts = [bool(v) for v in ok]
        return (verdicts, points_from_wire(pts, fl)) if points else verdicts

    def feldman_verify_dev(self, commitments, dealer, xs, shares, x_bits, ok_out, points_out=None, flags=None,
                           stream=None):
        """Device form: commitments (T, M, 64) uint8, dealer (n,) int32 or None, xs (n,) int32 (read as
        uint32), shares (n, 32) uint8 CUDA tensors -> ok_out (n,) uint8 and, unless None, points_out
        (n, 64) uint8 and flags (n,) int32; enqueued on `stream` (nothing staged or awaited).  A dealer
        index >= M is not checked here."""
        _need(commitments.dim() == 3 and shares.dim() == 2, "commitments must be (T, M, 64), shares (n, 32)")
        T, M, n = commitments.shape[0], commitments.shape[1], shares.shape[0]
        _dev_bytes(commitments, "commitments", 64, T * M)
        _dev_bytes(shares, "shares", 32, n)
        _dev_bytes(xs, "xs", 1, n, 4)
        _dev_bytes(ok_out, "ok_out", 1, n)
        if dealer is not None:
            _dev_bytes(dealer, "dealer", 1, n, 4)
        if points_out is not None:
            _dev_bytes(points_out, "points_out", 64, n)
        if flags is not None:
            _dev_bytes(flags, "flags", 1, n, 4)
        rc = self.lib.flm_feldman_verify_dev(self.ctx, _vp(commitments), T, M, _vp(dealer), _vp(xs), int(x_bits),
                                             _vp(shares), n, _vp(ok_out), _vp(points_out), _vp(flags),
                                             self._stream_handle(stream))
        self._check(rc, "flm_feldman_verify_dev")
        return ok_out

    def ec_combine_dev(self, c1, shares, lambdas, seeds_out, flags, points_out=None, negate: bool = True,
                       stream=None):
        """Device form: c1 (D,64), shares (T,D,64), lambdas (T,32) uint8 CUDA tensors;
        seeds_out (D,32) uint8 and flags (D,) int32 CUDA tensors are written on `stream`."""
        _need(shares.dim() == 3, "shares must be (T, D, 64)")
        T, D = shares.shape[0], shares.shape[1]
        _dev_bytes(shares, "shares", 64, T * D)
        _dev_bytes(lambdas, "lambdas", 32, T)
        if c1 is not None:
            _dev_bytes(c1, "c1", 64, D)
        if seeds_out is not None:
            _dev_bytes(seeds_out, "seeds_out", 32, D)
        if points_out is not None:
            _dev_bytes(points_out, "points_out", 64, D)
        _dev_bytes(flags, "flags", 1, D, 4)
        rc = self.lib.flm_ec_combine_dev(self.ctx, _vp(c1), _vp(shares), _vp(lambdas), T, D, 1 if negate else 0,
                                         _vp(points_out), _vp(seeds_out), _vp(flags), self._stream_handle(stream))
        self._check(rc, "flm_ec_combine_dev")
        return seeds_out

    def pair_units_dev(self, seeds, signs, dst, L: int, ws, groups: int, p0=None, p1=None, final: bool = False,
                       stream=None):
        """Pair masks as a shared work queue (flm_pair_units_dev): seeds (K,32) uint8, signs (K,) int8,
        dst (>= L) int32, ws (>= 2) int32 CUDA tensors.  final=False adds the units claimed before
        ws[1] is set into dst; final=True writes dst = p0 + p1 plus the units left."""
        K = seeds.shape[0] if seeds is not None else 0
        if K:
            _dev_bytes(seeds, "seeds", 32, K)
            _dev_bytes(signs, "signs", 1, K)
        _dev_bytes(dst, "dst", 1, L, 4)
        _dev_bytes(ws, "ws", 1, 2, 4)
        for name, t in (("p0", p0), ("p1", p1)):
            if t is not None:
                _dev_bytes(t, name, 1, L, 4)
        rc = self.lib.flm_pair_units_dev(self.ctx, _vp(seeds), _vp(signs), K, _vp(p0), _vp(p1), _vp(dst), L, _vp(ws),
                                         1 if final else 0, int(groups), self._stream_handle(stream))
        self._check(rc, "flm_pair_units_dev")
        return dst

    def flag_set_dev(self, ws, stream=None):
        """ws[1] = 1 once the work enqueued before it on `stream` is done (flm_flag_set_dev)."""
        self._check(self.lib.flm_flag_set_dev(self.ctx, ctypes.c_void_p(ws.data_ptr()), self._stream_handle(stream)),
                    "flm_flag_set_dev")

    def check_signs(self) -> int:
        bad = ctypes.c_int()
        self._check(self.lib.flm_check_signs(self.ctx, ctypes.byref(bad)), "flm_check_signs")
        return bad.value


class PinnedArena:
    """Page-locked host memory (hipHostMalloc) viewed as numpy arrays.

    Client vectors allocated here reach the GPU by DMA at the full PCIe rate
    (the reference keeps them as pageable numpy arrays, SA_ServiceAgent.py:210)."""

    def __init__(self, nbytes: int):
        self.lib = _lib.load()
        self.ptr = self.lib.flm_host_alloc(nbytes)
        if not self.ptr:
            raise RuntimeError(f"flm_host_alloc({nbytes}) failed")
        self.nbytes = nbytes
        self.off = 0

    def array(self, shape, dtype=np.uint32) -> np.ndarray:
        dt = np.dtype(dtype)
        n = int(np.prod(shape)) * dt.itemsize
        off = (self.off + 255) // 256 * 256
        if off + n > self.nbytes:
            raise RuntimeError("pinned arena exhausted")
        self.off = off + n
        buf = (ctypes.c_uint8 * n).from_address(self.ptr + off)
        return np.frombuffer(buf, dtype=dt).reshape(shape)

    def free(self):
        if self.ptr:
            self.lib.flm_host_free(self.ptr)
            self.ptr = None


# ------------------------------------------------------------------ multi-GPU
def rccl_available():
    """(True, "") when RCCL loads and resolves (flm_rccl_available; local, no GPU work), else (False, why)."""
    lib = _lib.load()
    if lib.flm_rccl_available():
        return True, ""
    return False, lib.flm_last_error(None).decode()


def comm_unique_id() -> bytes:
    """A fresh 128-byte RCCL unique id (flm_comm_unique_id), for rank 0 to broadcast."""
    lib = _lib.load()
    buf = (ctypes.c_uint8 * 128)()
    rc = lib.flm_comm_unique_id(buf)
    if rc != 0:
        raise RuntimeError(f"flm_comm_unique_id: {lib.flm_last_error(None).decode()}")
    return bytes(buf)


def shard_bounds(L: int, n_ranks: int, rank: int):
    """(lo, hi, S): rank's output slots [lo, hi) and the shard length S (flm_shard_bounds)."""
    lib = _lib.load()
    lo, hi, S = ctypes.c_size_t(), ctypes.c_size_t(), ctypes.c_size_t()
    if lib.flm_shard_bounds(int(L), int(n_ranks), int(rank), ctypes.byref(lo), ctypes.byref(hi), ctypes.byref(S)):
        raise RuntimeError("flm_shard_bounds: bad arguments")
    return lo.value, hi.value, S.value


def client_bounds(N: int, n_ranks: int, rank: int):
    """[c0, c1): the clients rank ingests (flm_client_bounds)."""
    lib = _lib.load()
    c0, c1 = ctypes.c_int(), ctypes.c_int()
    if lib.flm_client_bounds(int(N), int(n_ranks), int(rank), ctypes.byref(c0), ctypes.byref(c1)):
        raise RuntimeError("flm_client_bounds: bad arguments")
    return c0.value, c1.value


class DeviceGroup:
    """All GPUs of the node from ONE process (flm_group): the drop-in server's multi-GPU form.

    The reference server is a single-threaded DES process (Kernel.py:190-271); a group gives
    its report/reconstruction steps every device: client-sharded upload and row sum,
    slot-sharded unmask, one RCCL reduce-scatter (ncclUint32), shards back to the host.
    devices: distinct ids (RCCL clique) or one id repeated (loopback ranks on one GPU).
    force_rccl: give a one-device group an RCCL clique too (FLM_GROUP_RCCL), so its rounds take
    the multi-GPU path -- partial buffer, grouped ncclReduceScatter, shard -- on a one-GPU box."""

    def __init__(self, devices, force_rccl: bool = False):
        self.lib = _lib.load()
        if isinstance(devices, int):
            devices = list(range(devices))
        devices = [int(d) for d in devices]
        arr = (ctypes.c_int * len(devices))(*devices)
        g = ctypes.c_void_p()
        rc = self.lib.flm_group_init_flags(ctypes.byref(g), len(devices), arr, 1 if force_rccl else 0)
        if rc != 0:
            raise RuntimeError(f"flm_group_init({devices}): {self.lib.flm_group_last_error(None).decode()}")
        self.g = g
        self.devices = devices
        self.n = len(devices)
        self.loopback = bool(self.lib.flm_group_is_loopback(g))
        self.rccl = bool(self.lib.flm_group_has_rccl(g))
        self.force_rccl = bool(force_rccl)  # as requested (a group of distinct devices has a clique anyway)
        self._stores = 0                    # live VectorStores on this group (close() refuses while > 0)
        self.retired = False                # replaced while a store still used it: its last store closes it
        self.engines = [MaskEngine(d, _ctx=self.lib.flm_group_ctx(g, r)) for r, d in enumerate(devices)]

    def close(self):
        """Free the group.  Refused while a VectorStore created on it is still open: the store holds
        the group's contexts and streams (close the stores first)."""
        if getattr(self, "g", None) is not None and self.g.value:
            if self._stores:
                raise RuntimeError(f"DeviceGroup.close: {self._stores} VectorStore(s) still use this group")
            for e in self.engines:
                e.close()
            self.lib.flm_group_free(self.g)
            self.g = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _check(self, rc: int, what: str):
        if rc != 0:
            raise RuntimeError(f"{what}: {self.lib.flm_group_last_error(self.g).decode()} (code {rc})")

    def sync(self):
        self._check(self.lib.flm_group_sync(self.g), "flm_group_sync")

    def aggregate_unmask(self, vectors, seeds, signs, L: int | None = None) -> np.ndarray:
        """MaskEngine.aggregate_unmask over every device of the group (host rows in, host out)."""
        if isinstance(vectors, np.ndarray) and vectors.ndim == 2:
            rows = [np.ascontiguousarray(vectors[i], dtype=np.uint32) for i in range(vectors.shape[0])]
        else:
            rows = [np.ascontiguousarray(v, dtype=np.uint32) for v in vectors]
        if L is None:
            if not rows:
                raise RuntimeError("L is required when there are no vectors")
            L = rows[0].shape[0]
        for v in rows:
            if v.shape[0] != L:
                raise RuntimeError("Client sends vector of incorrect length.")  # SA_ServiceAgent.py:348-349
        seeds = _seeds_array(seeds)
        signs = _signs_array(signs, seeds.shape[0])
        out = np.empty(L, dtype=np.uint32)
        ptrs = (_lib._u32p * max(1, len(rows)))(*[p_u32(v) for v in rows])
        self._check(self.lib.flm_group_aggregate_unmask(self.g, ptrs, len(rows), p_u8(seeds), p_i8(signs),
                                                        seeds.shape[0], L, p_u32(out)),
                    "flm_group_aggregate_unmask")
        return out

    def rank_stream(self, r: int):
        """Rank r's context stream (flm_ctx_stream) as a torch ExternalStream: the group's rounds run there."""
        import torch
        cache = self.__dict__.setdefault("_rank_streams", {})
        if r not in cache:
            h = self.lib.flm_ctx_stream(self.lib.flm_group_ctx(self.g, r))
            cache[r] = torch.cuda.ExternalStream(h, device=torch.device("cuda", self.devices[r]))
        return cache[r]

    def wait(self):
        """Make torch's current stream on every rank's device wait for that rank's round
        (no host synchronisation): the shards can then be read in stream order."""
        import torch
        for r, d in enumerate(self.devices):
            torch.cuda.current_stream(torch.device("cuda", d)).wait_stream(self.rank_stream(r))

    def aggregate_unmask_dev(self, rows, seeds, signs, shards, L: int, after_current: bool = True):
        """rows/seeds/signs/shards: per-rank CUDA tensors on the ranks' devices (rows (N_r, pitch) with one
        common pitch; shards >= S words).  Enqueued on the ranks' context streams and returns.
        after_current: each rank's stream first waits for torch's current stream on its device, where
        the inputs were produced (False: the caller has ordered them itself).  Read the shards after
        sync() (host) or wait() (torch's current streams)."""
        n = self.n
        _need(len(rows) == n and len(shards) == n and len(seeds) == n and len(signs) == n,
              f"rows, seeds, signs and shards need one entry per rank ({n})")
        pitches = {_dev_rows(r, L) for r in rows if r is not None and r.shape[0]}
        _need(len(pitches) <= 1, f"every rank's rows need the same pitch, got {sorted(pitches)}")
        pitch = pitches.pop() if pitches else 0
        K = seeds[0].shape[0] if seeds and seeds[0] is not None else 0
        S = shard_bounds(L, n, 0)[2]
        for r in range(n):
            if K:
                _dev_bytes(seeds[r], f"seeds[{r}]", 32, K)
                _need(seeds[r].shape[0] == K, "every rank needs the same K seeds")
                _dev_bytes(signs[r], f"signs[{r}]", 1, K)
            _dev_bytes(shards[r], f"shards[{r}]", 1, S, 4)
        vp = ctypes.c_void_p
        d_rows = (vp * n)(*[r.data_ptr() if r is not None and r.shape[0] else 0 for r in rows])
        n_rows = (ctypes.c_int * n)(*[int(r.shape[0]) if r is not None else 0 for r in rows])
        d_seeds = (vp * n)(*[s.data_ptr() if K else 0 for s in seeds])
        d_signs = (vp * n)(*[s.data_ptr() if K else 0 for s in signs])
        d_shards = (vp * n)(*[s.data_ptr() for s in shards])
        if after_current:
            import torch
            for r, d in enumerate(self.devices):
                self.rank_stream(r).wait_stream(torch.cuda.current_stream(torch.device("cuda", d)))
        self._check(self.lib.flm_group_aggregate_unmask_dev(self.g, d_rows, pitch, n_rows, d_seeds, d_signs, K, L,
                                                            d_shards), "flm_group_aggregate_unmask_dev")
        return shards
