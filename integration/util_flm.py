"""util/flm.py for the reference tree: the ctypes binding a maintainer adds to eniac/flamingo.

Save as ``util/flm.py`` in the reference, then edit the call sites as INTEGRATION.md shows
(agent/flamingo/SA_ServiceAgent.py:346-350, 506-605; SA_ClientAgent.py:246-324).  It binds
libflamingo_hip.so directly -- no dependency on the flamingo_amd package -- and mirrors the
reference's own conventions: uint32 numpy vectors, 32-byte seeds, +-1 signs, EccPoint-like
objects with .x/.y for the ElGamal and decryption-share points, RuntimeError on failure
(as SA_ServiceAgent.py:349,502,579,592 raise).

Environment:
  FLM_LIB      path of libflamingo_hip.so (default: found by the dynamic loader)
  FLM_DEVICE   the GPU of the single-device context (default 0)
  FLM_GPUS     > 1: the server's aggregate_unmask runs on devices 0..FLM_GPUS-1 of this one
               process (flm_group: client-sharded rows, slot-sharded masks, one RCCL
               reduce-scatter, ncclUint32) -- the reference server is a single DES process
               (Kernel.py:190-271), so this is how it uses all GPUs of the node.
The contexts are created lazily, on first use: after SA_ServiceAgent.py:562 forks its
multiprocessing.Pool, never before.
"""
import ctypes
import os

import numpy as np

_lib = ctypes.CDLL(os.environ.get("FLM_LIB", "libflamingo_hip.so"))
_vp, _int, _sz = ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t
_u8p, _i8p, _u32p, _i64p = (ctypes.POINTER(t) for t in (ctypes.c_uint8, ctypes.c_int8, ctypes.c_uint32,
                                                         ctypes.c_int64))
_f32p = ctypes.POINTER(ctypes.c_float)
for _name, _res, _args in (
        ("flm_init", _int, [ctypes.POINTER(_vp), _int]),
        ("flm_last_error", ctypes.c_char_p, [_vp]),
        ("flm_aggregate_unmask", _int, [_vp, ctypes.POINTER(_u32p), _int, _u8p, _i8p, _int, _sz, _u32p]),
        ("flm_client_mask", _int, [_vp, _u32p, _int, _i64p, _u8p, _i8p, _sz, _u32p]),
        ("flm_shamir_combine", _int, [_vp, _u8p, _u8p, _int, _int, _u8p]),
        ("flm_shamir_deal", _int, [_vp, _u8p, _int, _int, _u32p, _int, _u8p]),
        ("flm_aes_gcm_xor", _int, [_vp, _u8p, _u8p, _int, _u8p, _u8p, _sz, _int]),
        ("flm_aes_gcm_seal", _int, [_vp, _u8p, _u8p, _int, _u8p, _sz, _u8p, _u8p, _sz, _u8p, _int]),
        ("flm_aes_gcm_open", _int, [_vp, _u8p, _u8p, _int, _u8p, _sz, _u8p, _u8p, _u8p, _sz, _u8p, _int]),
        ("flm_ecdsa_verify", _int, [_vp, _u8p, _u8p, _u8p, _int, _u8p, ctypes.POINTER(ctypes.c_uint32)]),
        ("flm_feldman_verify", _int, [_vp, _u8p, _int, _int, _u32p, _u32p, _int, _u8p, _int, _u8p, _u8p, _u32p]),
        ("flm_ec_combine", _int, [_vp, _u8p, _u8p, _u8p, _int, _int, _int, _u8p, _u8p, ctypes.POINTER(ctypes.c_uint32)]),
        ("flm_group_init", _int, [ctypes.POINTER(_vp), _int, ctypes.POINTER(_int)]),
        ("flm_group_last_error", ctypes.c_char_p, [_vp]),
        ("flm_group_aggregate_unmask", _int, [_vp, ctypes.POINTER(_u32p), _int, _u8p, _i8p, _int, _sz, _u32p]),
        ("flm_store_create", _int, [ctypes.POINTER(_vp), _vp, _vp, _sz, _int]),
        ("flm_store_free", None, [_vp]),
        ("flm_store_last_error", ctypes.c_char_p, [_vp]),
        ("flm_store_add", _int, [_vp, ctypes.c_int64, _vp, _sz]),
        ("flm_store_partial", _int, [_vp]),
        ("flm_store_unmask", _int, [_vp, _u8p, _i8p, _int, _u32p]),
        ("flm_store_unmask_f32", _int, [_vp, _u8p, _i8p, _int, _int, ctypes.c_int64, _f32p]),
        ("flm_store_reset", _int, [_vp]),
        ("flm_codec_check", _int, [_int, ctypes.c_float, ctypes.c_int64]),
        ("flm_client_encode_mask", _int, [_vp, _f32p, _int, _i64p, _u8p, _i8p, _sz, _int, ctypes.c_float, _u8p, _u32p,
                                          _u32p]),
        ("flm_decode_sum", _int, [_vp, _u32p, _sz, _int, ctypes.c_int64, _f32p]),
        ("flm_codec_check_packed", _int, [_int, ctypes.c_float, _int, ctypes.c_int64]),
        ("flm_client_encode_pack_mask", _int, [_vp, _f32p, _int, _i64p, _u8p, _i8p, _sz, _int, ctypes.c_float, _int, _u8p,
                                               _u32p, _u32p]),
        ("flm_decode_unpack", _int, [_vp, _u32p, _sz, _int, ctypes.c_float, _int, ctypes.c_int64, _f32p]),
        ("flm_store_unmask_unpack_f32", _int, [_vp, _u8p, _i8p, _int, _sz, _int, ctypes.c_float, _int, ctypes.c_int64,
                                               _f32p]),
        ("flm_codec_check_noise", _int, [_int, ctypes.c_float, _int, _int, ctypes.c_int64, ctypes.c_uint64]),
        ("flm_client_encode_noise_mask", _int, [_vp, _f32p, _int, _i64p, _u8p, _i8p, _sz, _int, ctypes.c_float, _int, _u8p,
                                                _int, _u8p, _u32p, _u32p]),
        ("flm_decode_unpack_noise", _int, [_vp, _u32p, _sz, _int, ctypes.c_float, _int, _int, ctypes.c_int64, _f32p]),
        ("flm_store_unmask_unpack_noise_f32", _int, [_vp, _u8p, _i8p, _int, _sz, _int, ctypes.c_float, _int, _int,
                                                     ctypes.c_int64, _f32p]),
        ("flm_codec_check_gauss", _int, [_int, ctypes.c_float, _int, _int, ctypes.c_int64, ctypes.c_uint64]),
        ("flm_codec_check_modular", _int, [_int, ctypes.c_float, _int, _int, ctypes.c_int64]),
        ("flm_decode_unpack_mod", _int, [_vp, _u32p, _sz, _int, ctypes.c_float, _int, _int, ctypes.c_int64, _int, _f32p,
                                         _u32p]),
        ("flm_store_unmask_unpack_mod_f32", _int, [_vp, _u8p, _i8p, _int, _sz, _int, ctypes.c_float, _int, _int,
                                                   ctypes.c_int64, _int, _f32p, _u32p]),
        ("flm_client_encode_gauss_mask", _int, [_vp, _f32p, _int, _i64p, _u8p, _i8p, _sz, _int, ctypes.c_float, _int, _u8p,
                                                _int, ctypes.POINTER(ctypes.c_uint64), _u8p, _u32p, _u32p]),
        ("flm_rotate_check", _int, [ctypes.c_uint64, _int, ctypes.POINTER(ctypes.c_uint64)]),
        ("flm_rotate", _int, [_vp, _f32p, _int, _sz, _int, _u8p, _int, _f32p, _u32p]),
        ("flm_l2_clip_check", _int, [ctypes.c_uint64, ctypes.c_float, _int, ctypes.POINTER(ctypes.c_uint64)]),
        ("flm_l2_clip", _int, [_vp, _f32p, _int, _sz, ctypes.c_float, _f32p, _f32p, ctypes.POINTER(ctypes.c_double)]),
        ("flm_rotate_clip", _int, [_vp, _f32p, _int, _sz, _int, _u8p, ctypes.c_float, _f32p, _u32p, _f32p,
                                   ctypes.POINTER(ctypes.c_double)]),
        ("flm_hash_to_curve", _int, [_vp, _u8p, _u32p, _int, _u8p, _u32p]),
        ("flm_hash_to_curve_decimal", _int, [_vp, ctypes.c_uint32, _int, _u8p, _u32p])):
    _f = getattr(_lib, _name)
    _f.restype, _f.argtypes = _res, _args

_ctx = None
_group = None


def _context():
    global _ctx
    if _ctx is None:
        c = _vp()
        if _lib.flm_init(ctypes.byref(c), int(os.environ.get("FLM_DEVICE", "0"))):
            raise RuntimeError(_lib.flm_last_error(None).decode())
        _ctx = c
    return _ctx


def _server_group():
    """The process's device group when FLM_GPUS > 1, else None."""
    global _group
    n = int(os.environ.get("FLM_GPUS", "1"))
    if n <= 1:
        return None
    if _group is None:
        g = _vp()
        if _lib.flm_group_init(ctypes.byref(g), n, None):
            raise RuntimeError(_lib.flm_group_last_error(None).decode())
        _group = g
    return _group


def _check(rc, group=None):
    if rc:
        msg = _lib.flm_group_last_error(group) if group is not None else _lib.flm_last_error(_ctx)
        raise RuntimeError(msg.decode())


def _u32_body(vec, L):
    """A VECTOR body as contiguous uint32[L], or None when it is not a 1-D 32-bit integer vector of
    length L: the reference's `vec_sum_partial += v` (SA_ServiceAgent.py:346-350) raises on such a
    body (wrong length at :348-349; numpy's same-kind cast refuses float and 64-bit bodies), so it
    is never silently truncated into one."""
    v = np.asarray(vec)
    if v.ndim != 1 or v.shape[0] != L or v.dtype.kind not in "ui" or v.dtype.itemsize != 4:
        return None
    return np.ascontiguousarray(v).view(np.uint32)


def _seed_arrays(seeds, signs):
    K = len(seeds)
    sd = np.frombuffer(b"".join(bytes(s) for s in seeds), np.uint8) if K else np.zeros(32, np.uint8)
    sg = np.asarray(signs, np.int8) if K else np.ones(1, np.int8)
    if sd.size != 32 * K or sg.size != max(K, 1):
        raise RuntimeError("seeds must be 32 bytes each, one sign per seed")
    return sd, sg, K


def aggregate_unmask(vectors, seeds, signs, L):
    """sum(vectors) + sum_k signs[k] * PRG(seeds[k]) mod 2^32, as uint32[L]
    (vec_sum_partial + cancel_vec + mi_vec, SA_ServiceAgent.py:346-350, 529-605)."""
    vecs = [_u32_body(v, L) for v in vectors]
    if any(v is None for v in vecs):
        raise RuntimeError("Client sends vector of incorrect length.")
    rows = (_u32p * max(1, len(vecs)))(*[v.ctypes.data_as(_u32p) for v in vecs])
    sd, sg, K = _seed_arrays(seeds, signs)
    out = np.empty(L, np.uint32)
    g = _server_group()
    if g is not None:
        _check(_lib.flm_group_aggregate_unmask(g, rows, len(vecs), sd.ctypes.data_as(_u8p), sg.ctypes.data_as(_i8p),
                                               K, L, out.ctypes.data_as(_u32p)), g)
    else:
        _check(_lib.flm_aggregate_unmask(_context(), rows, len(vecs), sd.ctypes.data_as(_u8p),
                                         sg.ctypes.data_as(_i8p), K, L, out.ctypes.data_as(_u32p)))
    return out


def _be(ints):
    """Python ints -> n x 32 big-endian bytes."""
    return np.frombuffer(b"".join(int(v).to_bytes(32, "big") for v in ints), np.uint8)


def shamir_combine(shares_by_member, coeffs):
    """[(sum_j coeffs[j] * shares_by_member[j][i]) % n .to_bytes(32, 'big') for each i]
    (the m_i recovery of SA_ServiceAgent.py:517-526)."""
    T, M = len(coeffs), len(shares_by_member[0])
    sh = np.concatenate([_be(s) for s in shares_by_member])
    out = np.empty(M * 32, np.uint8)
    _check(_lib.flm_shamir_combine(_context(), sh.ctypes.data_as(_u8p), _be(coeffs).ctypes.data_as(_u8p), T, M,
                                   out.ctypes.data_as(_u8p)))
    return [out[32 * i:32 * i + 32].tobytes() for i in range(M)]


def shamir_deal(coeffs_by_term, xs):
    """[[sum_j coeffs_by_term[j][i] * x^j % n for each secret i] for x in xs]: the dealing of
    SA_ClientAgent.py:218-220 (secret_int_to_points) for a batch of clients, term 0 the secrets
    (any value below 2^256), xs the non-zero evaluation points (the reference's 1..num_points)."""
    T, M, C = len(coeffs_by_term), len(coeffs_by_term[0]), len(xs)
    co = np.concatenate([_be(c) for c in coeffs_by_term]) if M else np.zeros(32, np.uint8)
    x = np.asarray([int(v) for v in xs], np.uint32)
    out = np.empty(max(1, C * M * 32), np.uint8)
    _check(_lib.flm_shamir_deal(_context(), co.ctypes.data_as(_u8p), T, M, x.ctypes.data_as(_u32p), C,
                                out.ctypes.data_as(_u8p)))
    return [[int.from_bytes(out[32 * (c * M + i):32 * (c * M + i) + 32].tobytes(), "big") for i in range(M)]
            for c in range(C)]


def aes_gcm_xor(keys, nonces, datas):
    """[AES.new(key, AES.MODE_GCM, nonce=nonce).encrypt(data)] for a batch of equally long messages
    (at most 256 bytes) and equally long nonces (12 or 16 bytes), tags dropped: the per-share
    encryption of SA_ClientAgent.py:227-244 and, being the same XOR, the decryption of :402-420."""
    n = len(datas)
    if n == 0:
        return []
    k, nc, d = (np.frombuffer(b"".join(bytes(v) for v in part), np.uint8) for part in (keys, nonces, datas))
    ln, nl = len(datas[0]), len(nonces[0])
    if k.size != 16 * n or nc.size != nl * n or d.size != ln * n:
        raise RuntimeError("keys must be 16 bytes each; nonces, and messages, of one length")
    out = np.empty(ln * n, np.uint8)
    _check(_lib.flm_aes_gcm_xor(_context(), k.ctypes.data_as(_u8p), nc.ctypes.data_as(_u8p), nl,
                                d.ctypes.data_as(_u8p), out.ctypes.data_as(_u8p), ln, n))
    return [out[ln * i:ln * i + ln].tobytes() for i in range(n)]


def _gcm_batch(keys, nonces, aads, datas):
    n = len(datas)
    k, nc, d = (np.frombuffer(b"".join(bytes(v) for v in part), np.uint8) for part in (keys, nonces, datas))
    ln, nl = len(datas[0]), len(nonces[0])
    al = len(aads[0]) if aads else 0
    a = np.frombuffer(b"".join(bytes(v) for v in aads), np.uint8) if al else None
    if k.size != 16 * n or nc.size != nl * n or d.size != ln * n or (al and (len(aads) != n or a.size != al * n)):
        raise RuntimeError("keys must be 16 bytes each; nonces, messages, and AADs, of one length")
    return n, k, nc, nl, a, al, d, ln


def aes_gcm_seal(keys, nonces, datas, aads=None):
    """[(ct, tag)] with c = AES.new(key, AES.MODE_GCM, nonce=nonce); c.update(aad); ct, tag =
    c.encrypt_and_digest(data), for a batch of equally long messages (at most 256 bytes), nonces (12
    or 16 bytes) and AADs (at most 64 bytes, or None): the sealing of SA_ClientAgent.py:227-244 with
    the tag the reference discards at :242."""
    if len(datas) == 0:
        return []
    n, k, nc, nl, a, al, d, ln = _gcm_batch(keys, nonces, aads, datas)
    out, tags = np.empty(max(1, ln * n), np.uint8), np.empty(16 * n, np.uint8)
    _check(_lib.flm_aes_gcm_seal(_context(), k.ctypes.data_as(_u8p), nc.ctypes.data_as(_u8p), nl,
                                 a.ctypes.data_as(_u8p) if al else None, al, d.ctypes.data_as(_u8p),
                                 out.ctypes.data_as(_u8p), ln, tags.ctypes.data_as(_u8p), n))
    return [(out[ln * i:ln * i + ln].tobytes(), tags[16 * i:16 * i + 16].tobytes()) for i in range(n)]


def aes_gcm_open(keys, nonces, cts, tags, aads=None):
    """[c.decrypt_and_verify(ct, tag), or None where it raises ValueError("MAC check failed")] for a
    batch: the opening of SA_ClientAgent.py:402-425 with the check it leaves out."""
    if len(cts) == 0:
        return []
    n, k, nc, nl, a, al, d, ln = _gcm_batch(keys, nonces, aads, cts)
    t = np.frombuffer(b"".join(bytes(v) for v in tags), np.uint8)
    if t.size != 16 * n:
        raise RuntimeError("tags must be 16 bytes each")
    out, ok = np.empty(max(1, ln * n), np.uint8), np.zeros(n, np.uint8)
    _check(_lib.flm_aes_gcm_open(_context(), k.ctypes.data_as(_u8p), nc.ctypes.data_as(_u8p), nl,
                                 a.ctypes.data_as(_u8p) if al else None, al, d.ctypes.data_as(_u8p),
                                 t.ctypes.data_as(_u8p), out.ctypes.data_as(_u8p), ln, ok.ctypes.data_as(_u8p), n))
    return [out[ln * i:ln * i + ln].tobytes() if ok[i] else None for i in range(n)]


def ecdsa_verify(public_keys, messages, signatures):
    """[DSS.new(key, 'fips-186-3').verify(SHA256.new(msg), sig) succeeded] for a batch: the check
    SA_ClientAgent.py:387 leaves as `# CHECK SIGNATURES`, over the server's signature of the offline
    set and the committee signatures it forwards in DEC (SA_ServiceAgent.py:382-386).  public_keys:
    EccPoint-like objects (.x, .y), e.g. ECC.import_key(...).pointQ; messages: the signed bytes;
    signatures: 64 bytes r || s each.  A forged signature is a False in the list, not an exception."""
    import hashlib
    n = len(signatures)
    if n == 0:
        return []
    if len(public_keys) != n or len(messages) != n:
        raise RuntimeError("one public key and one message per signature")
    sg = np.zeros((n, 64), np.uint8)
    for i, s in enumerate(signatures):
        if len(s) == 64:                       # another length: r = s = 0, refused
            sg[i] = np.frombuffer(bytes(s), np.uint8)
    pk = _be([c for p in public_keys for c in (int(p.x), int(p.y))])
    dg = np.frombuffer(b"".join(hashlib.sha256(bytes(m)).digest() for m in messages), np.uint8)
    ok = np.zeros(n, np.uint8)
    _check(_lib.flm_ecdsa_verify(_context(), pk.ctypes.data_as(_u8p), dg.ctypes.data_as(_u8p),
                                 sg.ctypes.data_as(_u8p), n, ok.ctypes.data_as(_u8p), None))
    return [bool(v) for v in ok]


def feldman_verify(shares, ids, commitments_by_dealer):
    """[verify_commitment(s_ij, commitments of dealer i) as member j sees it] for a batch
    (agent/dkg/SA_ClientAgent.py:219-228): shares[r] * G == sum_k ids[r]**k * commitments_by_dealer[r][k],
    one row per (share, checking member's id, that dealer's commitment list) -- a member's n rows of
    SHARE_AND_COMMIT (:93-96, every id its own) or the broadcast shares of FORWARD_SHARE (:141-146).
    shares: integers (the y of the (x, y) tuples); commitments: EccPoint-like objects (.x, .y), with
    EccPoint(0, 0) the point at infinity.  A failed check is a False in the list, not an exception."""
    n = len(shares)
    if n == 0:
        return []
    if len(ids) != n or len(commitments_by_dealer) != n:
        raise RuntimeError("one id and one commitment list per share")
    T = len(commitments_by_dealer[0])
    if any(len(c) != T for c in commitments_by_dealer):
        raise RuntimeError("every commitment list must have the same length")
    com = _be([v for k in range(T) for c in commitments_by_dealer for v in (int(c[k].x), int(c[k].y))])  # term-major
    sh = np.full((n, 32), 0xFF, np.uint8)          # a share outside [0, 2^256): refused like any share >= n
    for i, s in enumerate(shares):
        if 0 <= int(s) < (1 << 256):
            sh[i] = np.frombuffer(int(s).to_bytes(32, "big"), np.uint8)
    xs = np.array([int(v) for v in ids], np.uint32)
    ok = np.zeros(n, np.uint8)
    _check(_lib.flm_feldman_verify(_context(), com.ctypes.data_as(_u8p), T, n, None, xs.ctypes.data_as(_u32p),
                                   max(1, int(xs.max()).bit_length()), sh.ctypes.data_as(_u8p), n,
                                   ok.ctypes.data_as(_u8p), None, None))
    return [bool(v) for v in ok]


def ec_combine(c1_points, shares_by_member, coeffs):
    """SHA-256 keys of c1_i - sum_j coeffs[j] * shares_by_member[j][i] (SA_ServiceAgent.py:542-585):
    EccPoint-like objects (.x, .y) in, 32-byte ChaCha20 keys out."""
    xy = lambda pts: _be([c for p in pts for c in (int(p.x), int(p.y))])
    T, D = len(coeffs), len(c1_points)
    if D == 0:
        return []
    sh = np.concatenate([xy(s) for s in shares_by_member])
    seeds = np.empty(D * 32, np.uint8)
    _check(_lib.flm_ec_combine(_context(), xy(c1_points).ctypes.data_as(_u8p), sh.ctypes.data_as(_u8p),
                               _be(coeffs).ctypes.data_as(_u8p), T, D, 1, None, seeds.ctypes.data_as(_u8p), None))
    return [seeds[32 * i:32 * i + 32].tobytes() for i in range(D)]


class Point:
    """The .x / .y of pycryptodome's EccPoint, which is all SA_ClientAgent.py:288-289 and the
    ElGamal encryption (:434-447, via ECC.EccPoint(x, y)) read of a hash-to-curve result."""
    __slots__ = ("x", "y")

    def __init__(self, x, y):
        self.x, self.y = x, y


_h2c_table = None


def hash_str_to_curve(msg):
    """ecchash.hash_str_to_curve(msg, count=2, modulus=n, degree=1, blen=48, XMD SHA-256) as
    SA_ClientAgent.py:283-286 calls it, on the GPU.  The client's h_ijt is str(x & 0xFFFF) (:280):
    the first such call computes all 2^16 points in one launch (flm_hash_to_curve_decimal) and later
    calls index the table; any other message (<= 64 bytes) is one flm_hash_to_curve launch."""
    global _h2c_table
    if isinstance(msg, str) and msg.isdigit() and str(int(msg)) == msg and int(msg) < (1 << 16):
        if _h2c_table is None:
            out = np.empty((1 << 16, 64), np.uint8)
            fl = np.empty(1 << 16, np.uint32)
            _check(_lib.flm_hash_to_curve_decimal(_context(), 0, 1 << 16, out.ctypes.data_as(_u8p),
                                                  fl.ctypes.data_as(_u32p)))
            _h2c_table = (out, fl)
        row, f = _h2c_table[0][int(msg)], int(_h2c_table[1][int(msg)])
    else:
        m = msg.encode() if isinstance(msg, str) else bytes(msg)
        buf = np.zeros(64, np.uint8)
        buf[:len(m)] = np.frombuffer(m, np.uint8)
        out, fl, ln = np.empty(64, np.uint8), np.zeros(1, np.uint32), np.array([len(m)], np.uint32)
        _check(_lib.flm_hash_to_curve(_context(), buf.ctypes.data_as(_u8p), ln.ctypes.data_as(_u32p), 1,
                                      out.ctypes.data_as(_u8p), fl.ctypes.data_as(_u32p)))
        row, f = out, int(fl[0])
    if f & 4:
        return Point(0, 0)                   # the point at infinity, as pycryptodome's EccPoint(0, 0)
    b = row.tobytes()
    return Point(int.from_bytes(b[:32], "big"), int.from_bytes(b[32:], "big"))


def client_mask(seeds, signs, L, x=None):
    """x (default: the all-ones input of SA_ClientAgent.py:304) + sum_k signs[k] * PRG(seeds[k])
    for one client: the composition of SA_ClientAgent.py:246-324."""
    seg = np.array([0, len(seeds)], np.int64)
    sd, sg, K = _seed_arrays(seeds, signs)
    out = np.empty(L, np.uint32)
    xp = None
    if x is not None:
        x = np.ascontiguousarray(x, dtype=np.uint32)
        if x.shape != (L,):
            raise RuntimeError("vector length error")
        xp = x.ctypes.data_as(_u32p)
    _check(_lib.flm_client_mask(_context(), xp, 1, seg.ctypes.data_as(_i64p), sd.ctypes.data_as(_u8p),
                                sg.ctypes.data_as(_i8p), L, out.ctypes.data_as(_u32p)))
    return out


def codec_check(frac_bits, clip, n_clients):
    """Raise unless n_clients float updates of magnitude <= clip fit the 32-bit ring at frac_bits fractional
    bits (n ceil(clip 2^frac_bits) <= 2^31 - 1): the server's check at set-up, with the real n."""
    _check(_lib.flm_codec_check(int(frac_bits), float(clip), int(n_clients)))


def _encode_mask(fn, codec, seeds, signs, L, x, frac_bits, clip, pack, dither=None, noise=None):
    """One client's call of the encode entry point `fn`; codec(dither, noise): its arguments between clip and out,
    which is where the three entry points differ.  Returns (uint32[ceil(L / pack)], number of clipped elements)."""
    seg = np.array([0, len(seeds)], np.int64)
    sd, sg, K = _seed_arrays(seeds, signs)
    x = np.ascontiguousarray(x, dtype=np.float32)
    if x.shape != (L,):
        raise RuntimeError("vector length error")
    keep, ptrs = [], []
    for name, v in (("dither", dither), ("noise", noise)):
        if v is None:
            ptrs.append(None)
            continue
        if len(v) != 32:
            raise RuntimeError("the %s seed must be 32 bytes" % name)
        keep.append(np.frombuffer(bytes(v), np.uint8).copy())
        ptrs.append(keep[-1].ctypes.data_as(_u8p))
    out, clipped = np.empty(-(-L // pack), np.uint32), np.zeros(1, np.uint32)
    _check(fn(_context(), x.ctypes.data_as(_f32p), 1, seg.ctypes.data_as(_i64p), sd.ctypes.data_as(_u8p),
              sg.ctypes.data_as(_i8p), L, int(frac_bits), float(clip), *codec(*ptrs), out.ctypes.data_as(_u32p),
              clipped.ctypes.data_as(_u32p)))
    return out, int(clipped[0])


def client_encode_mask(seeds, signs, L, x, frac_bits, clip, dither=None):
    """client_mask for a float32 update x ("For machine learning, replace it with model weights",
    SA_ClientAgent.py:300-304): encode(x) + sum_k signs[k] * PRG(seeds[k]) with the fixed-point encoding
    (clip to +-clip, frac_bits fractional bits; nearest-even, or stochastic with a 32-byte dither seed) fused
    into the masking of SA_ClientAgent.py:304-324.  Returns (uint32[L], number of clipped elements)."""
    return _encode_mask(_lib.flm_client_encode_mask, lambda d, z: (d,), seeds, signs, L, x, frac_bits, clip, 1, dither)


def decode_sum(total, frac_bits, count=1):
    """final_sum (SA_ServiceAgent.py:538-540, 605) as the float32 mean of `count` contributors:
    float32(int32(total) / (count 2^frac_bits))."""
    total = np.ascontiguousarray(total, dtype=np.uint32)
    out = np.empty(total.shape[0], np.float32)
    _check(_lib.flm_decode_sum(_context(), total.ctypes.data_as(_u32p), total.shape[0], int(frac_bits), int(count),
                               out.ctypes.data_as(_f32p)))
    return out


def codec_check_packed(frac_bits, clip, pack, n_clients):
    """Raise unless n_clients float updates of magnitude <= clip fit `pack` (2 or 4) fields per ring word:
    n 2 ceil(clip 2^frac_bits) <= 2^(32 / pack) - 1, so that no field of the sum carries into its neighbour.
    The server's check at set-up, with the real n; pack = 4 serves small cohorts only (n <= 31 at 2 bits, clip 1)."""
    _check(_lib.flm_codec_check_packed(int(frac_bits), float(clip), int(pack), int(n_clients)))


def client_encode_pack_mask(seeds, signs, L, x, frac_bits, clip, pack, dither=None):
    """client_encode_mask with `pack` parameters per ring word ("replace it with model weights",
    SA_ClientAgent.py:300-304, masked as :304-324): the VECTOR body is ceil(L / pack) words, field j of word l'
    holding encode(x[pack l' + j]) + ceil(clip 2^frac_bits).  Returns (uint32[ceil(L / pack)], clipped elements)."""
    if pack not in (2, 4):
        raise RuntimeError("pack must be 2 or 4")
    return _encode_mask(_lib.flm_client_encode_pack_mask, lambda d, z: (int(pack), d), seeds, signs, L, x, frac_bits, clip,
                        pack, dither)


def decode_unpack(total, L, frac_bits, clip, pack, count=1, noise_bits=0):
    """final_sum of packed rows (SA_ServiceAgent.py:538-540, 605) as the L float32 means of `count`
    contributors: (field - count ceil(clip 2^frac_bits)) / (count 2^frac_bits).  noise_bits > 0: rows of
    client_encode_noise_mask, whose bias is ceil(clip 2^frac_bits) + noise_bits / 2."""
    if pack not in (2, 4):
        raise RuntimeError("pack must be 2 or 4")
    total = np.ascontiguousarray(total, dtype=np.uint32)
    if total.shape != (-(-L // pack),):
        raise RuntimeError("vector length error")
    out = np.empty(L, np.float32)
    _check(_lib.flm_decode_unpack_noise(_context(), total.ctypes.data_as(_u32p), L, int(frac_bits), float(clip),
                                        int(pack), int(noise_bits), int(count), out.ctypes.data_as(_f32p)))
    return out


def codec_check_modular(frac_bits, clip, pack, noise_bits, n_clients):
    """Raise unless a packed sum over n_clients can be decoded modulo the field (decode_unpack_mod): pack 2 or 4, one
    contributor's field fits, 2 (ceil(clip 2^frac_bits) + noise_bits / 2) <= 2^(32 / pack) - 1, and n_clients <=
    2^31 - 1.  The server's check at set-up in the place of codec_check_noise's worst case (SA_ServiceAgent.py:538-540,
    605); the table mode of the noise passes noise_bits = 2 tail."""
    _check(_lib.flm_codec_check_modular(int(frac_bits), float(clip), int(pack), int(noise_bits), int(n_clients)))


def decode_unpack_mod(total, L, frac_bits, clip, pack, count=1, noise_bits=0, guard=1):
    """decode_unpack of a final_sum taken modulo the field (SA_ServiceAgent.py:538-540, 605): every field a residue
    mod 2^(32 / pack), centred into [-H, H - 1], its carry followed into the field above.  Returns (float32[L], (near,
    max_abs)): the parameters whose centred sum has magnitude >= guard (an integer in 1..H), and the largest."""
    if pack not in (2, 4):
        raise RuntimeError("pack must be 2 or 4")
    total = np.ascontiguousarray(total, dtype=np.uint32)
    if total.shape != (-(-L // pack),):
        raise RuntimeError("vector length error")
    out, st = np.empty(L, np.float32), np.zeros(2, np.uint32)
    _check(_lib.flm_decode_unpack_mod(_context(), total.ctypes.data_as(_u32p), L, int(frac_bits), float(clip), int(pack),
                                      int(noise_bits), int(count), int(guard), out.ctypes.data_as(_f32p),
                                      st.ctypes.data_as(_u32p)))
    return out, (int(st[0]), int(st[1]))


def codec_check_noise(frac_bits, clip, pack, noise_bits, n_clients, L=0):
    """Raise unless n_clients float updates of magnitude <= clip, each with its share of binomial noise
    (noise_bits fair coins per parameter: at most noise_bits / 2 either way), fit the ring at `pack` (1, 2 or 4)
    parameters per word, in the worst case: n (ceil(clip 2^frac_bits) + noise_bits / 2) <= 2^31 - 1, packed twice
    that <= 2^(32 / pack) - 1; with L > 0 also ceil(noise_bits / 32) ceil(L / 16) <= 2^32.  The server's check at
    set-up, with the real n."""
    _check(_lib.flm_codec_check_noise(int(frac_bits), float(clip), int(pack), int(noise_bits), int(n_clients), int(L)))


def client_encode_noise_mask(seeds, signs, L, x, frac_bits, clip, pack=1, dither=None, noise_bits=0, noise=None):
    """client_encode_mask (pack 1) or client_encode_pack_mask (2, 4) with the client's share of distributed-DP
    noise drawn inside the masking kernel ("replace it with model weights", SA_ClientAgent.py:300-324; the local
    noise of agent/examples/crypto/PPFL_ClientAgent.py:219-221, 274-285): every parameter's quantised value gets
    (heads of noise_bits fair coins of PRG(noise)) - noise_bits / 2.  noise: 32 secret bytes, fresh per iteration.
    Turning noise_bits into an (epsilon, delta) is the caller's business.  Returns (uint32 words, clipped elements)."""
    if pack not in (1, 2, 4):
        raise RuntimeError("pack must be 1, 2 or 4")
    return _encode_mask(_lib.flm_client_encode_noise_mask, lambda d, z: (int(pack), d, int(noise_bits), z), seeds, signs, L,
                        x, frac_bits, clip, pack, dither, noise)


def codec_check_gauss(frac_bits, clip, pack, tail, n_clients, L=0):
    """codec_check_noise for table-sampled noise shares in [-tail, tail] (tail in 1..512): ceil(clip 2^frac_bits) +
    tail in the bound's place; with L > 0 also 2 ceil(L / 16) <= 2^32.  The server's check at set-up, with the real n."""
    _check(_lib.flm_codec_check_gauss(int(frac_bits), float(clip), int(pack), int(tail), int(n_clients), int(L)))


def client_encode_gauss_mask(seeds, signs, L, x, frac_bits, clip, table, noise, pack=1, dither=None):
    """client_encode_noise_mask with the client's noise share sampled from a cumulative table inside the masking kernel
    ("replace it with model weights", SA_ClientAgent.py:300-324; the local noise of
    agent/examples/crypto/PPFL_ClientAgent.py:219-221, 274-285): table 2 tail non-decreasing uint64 thresholds
    (flamingo_amd.dgauss.table builds a discrete Gaussian's), every parameter's quantised value gets (entries <= its
    64-bit draw of PRG(noise)) - tail.  noise: 32 secret bytes, fresh per iteration.  The rows decode with decode_sum
    (pack 1) or decode_unpack at noise_bits = 2 tail.  Returns (uint32 words, clipped elements)."""
    if pack not in (1, 2, 4):
        raise RuntimeError("pack must be 1, 2 or 4")
    table = np.ascontiguousarray(table, dtype=np.uint64)
    if table.ndim != 1 or table.shape[0] % 2:
        raise RuntimeError("table must hold 2 tail uint64 entries")
    cdt = table.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))
    return _encode_mask(_lib.flm_client_encode_gauss_mask, lambda d, z: (int(pack), d, table.shape[0] // 2, cdt, z), seeds,
                        signs, L, x, frac_bits, clip, pack, dither, noise)


def l2_clip_check(L, clip_norm, N=1):
    """Raise unless N updates of L parameters can be clipped to the L2 norm clip_norm (finite and positive; L > 0,
    N >= 1, at most 2^31 - 1 tiles of 4096 parameters in all); returns N ceil(L / 4096), the doubles of work space
    the device form takes.  No device call."""
    work = ctypes.c_uint64(0)
    if _lib.flm_l2_clip_check(int(L), float(clip_norm), int(N), ctypes.byref(work)):
        raise RuntimeError(_lib.flm_last_error(None).decode())
    return int(work.value)


def l2_clip(x, clip_norm):
    """One client's float32 update ("replace it with model weights", SA_ClientAgent.py:300-304) scaled to an L2 norm of
    at most clip_norm, in front of client_encode_*mask when no rotation is used: (x s, s, S) with S the sum of the
    squares in float64 (non-finite elements count as 0) and s = 1 if S <= clip_norm^2, else float32(clip_norm /
    sqrt(S)).  One client then moves the sum by at most clip_norm (1 + 2^-22) in L2."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    if x.ndim != 1:
        raise RuntimeError("vector length error")
    out, s, S = np.empty_like(x), np.zeros(1, np.float32), np.zeros(1, np.float64)
    _check(_lib.flm_l2_clip(_context(), x.ctypes.data_as(_f32p), 1, x.shape[0], float(clip_norm), out.ctypes.data_as(_f32p),
                            s.ctypes.data_as(_f32p), S.ctypes.data_as(ctypes.POINTER(ctypes.c_double))))
    return out, float(s[0]), float(S[0])


def rotate(x, key, log2_block, inverse=False, L=None, clip_norm=None):
    """The randomised block Hadamard rotation under the 32-byte public `key`, blocks of 2^log2_block parameters (4..12).
    Forward, the client's step in front of client_encode_*mask (SA_ClientAgent.py:300-304): x float32[L] ->
    (float32[L_rot], non-finite inputs zeroed), L_rot = L rounded up to whole blocks, which is then the L of the encode;
    with clip_norm the update is first scaled to that L2 norm in the same pass, as l2_clip does:
    (float32[L_rot], non-finite, s, S).  Inverse, the server's step behind decode_sum / decode_unpack
    (SA_ServiceAgent.py:538-540, 605): x float32[L_rot] and L, the length before the rotation -> float32[L]."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    if x.ndim != 1 or len(key) != 32:
        raise RuntimeError("one float32 vector and a 32-byte key")
    if inverse and (L is None or clip_norm is not None):
        raise RuntimeError("the inverse rotation takes L and no clip_norm")
    L = int(L) if inverse else x.shape[0]
    L_rot = ctypes.c_uint64(0)
    if _lib.flm_rotate_check(L, int(log2_block), ctypes.byref(L_rot)):
        raise RuntimeError(_lib.flm_last_error(None).decode())
    if inverse and x.shape[0] != L_rot.value:
        raise RuntimeError("vector length error")
    k = np.frombuffer(bytes(key), np.uint8).copy()
    out, bad = np.empty(L if inverse else L_rot.value, np.float32), np.zeros(1, np.uint32)
    if clip_norm is None:
        _check(_lib.flm_rotate(_context(), x.ctypes.data_as(_f32p), 1, L, int(log2_block), k.ctypes.data_as(_u8p),
                               int(bool(inverse)), out.ctypes.data_as(_f32p), None if inverse else bad.ctypes.data_as(_u32p)))
        return out if inverse else (out, int(bad[0]))
    s, S = np.zeros(1, np.float32), np.zeros(1, np.float64)
    _check(_lib.flm_rotate_clip(_context(), x.ctypes.data_as(_f32p), 1, L, int(log2_block), k.ctypes.data_as(_u8p),
                                float(clip_norm), out.ctypes.data_as(_f32p), bad.ctypes.data_as(_u32p),
                                s.ctypes.data_as(_f32p), S.ctypes.data_as(ctypes.POINTER(ctypes.c_double))))
    return out, int(bad[0]), float(s[0]), float(S[0])


class VectorStore:
    """The server's VECTOR bodies on the GPU(s) from arrival to final_sum (flm_store_*): hand each
    body to add() in receiveMessage (:205-210), call partial() in report_process (:346-350) and
    unmask() in reconstruction_process (:529-605), reset() when the pools are cleared (:488-497).
    On FLM_GPUS > 1 devices the rows are spread over the group and S stays slot-sharded."""

    def __init__(self, L, capacity):
        h = _vp()
        g = _server_group()
        if _lib.flm_store_create(ctypes.byref(h), None if g is not None else _context(), g, L, capacity):
            raise RuntimeError(_lib.flm_store_last_error(None).decode())
        self.h, self.L = h, L

    def _check(self, rc):
        if rc:
            raise RuntimeError(_lib.flm_store_last_error(self.h).decode())

    def close(self):
        """Free the store's device rows and pinned staging ring (flm_store_free)."""
        if getattr(self, "h", None) is not None and self.h.value:
            _lib.flm_store_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def add(self, sender, vec):
        """A body that is not a uint32[L]-compatible vector is remembered as bad: partial() then
        raises, as report_process does (:348-349)."""
        v = _u32_body(vec, self.L)
        if v is None:
            self._check(_lib.flm_store_add(self.h, int(sender), None, 0))
            return
        self._check(_lib.flm_store_add(self.h, int(sender), v.ctypes.data, self.L))

    def partial(self):
        """S = sum of the stored vectors, left on the GPU(s); raises on a body of the wrong length
        (:348-349)."""
        self._check(_lib.flm_store_partial(self.h))

    def unmask(self, seeds, signs):
        """final_sum = S + sum_k signs[k] * PRG(seeds[k]) as uint32[L] (:538-540, :605)."""
        sd, sg, K = _seed_arrays(seeds, signs)
        out = np.empty(self.L, np.uint32)
        self._check(_lib.flm_store_unmask(self.h, sd.ctypes.data_as(_u8p), sg.ctypes.data_as(_i8p), K,
                                          out.ctypes.data_as(_u32p)))
        return out

    def unmask_f32(self, seeds, signs, frac_bits, count=1):
        """unmask() decoded on the GPU(s) before the copy to the host: the float32 mean of `count`
        contributors (:538-540, :605, and the codec of client_encode_mask)."""
        sd, sg, K = _seed_arrays(seeds, signs)
        out = np.empty(self.L, np.float32)
        self._check(_lib.flm_store_unmask_f32(self.h, sd.ctypes.data_as(_u8p), sg.ctypes.data_as(_i8p), K,
                                              int(frac_bits), int(count), out.ctypes.data_as(_f32p)))
        return out

    def unmask_unpack_f32(self, seeds, signs, L_params, frac_bits, clip, pack, count=1, noise_bits=0):
        """unmask() of a store of packed rows (L = ceil(L_params / pack)), decoded on the GPU(s) before the copy
        to the host: the L_params float32 means of `count` contributors (:538-540, :605, and the codec of
        client_encode_pack_mask; noise_bits > 0: of client_encode_noise_mask)."""
        sd, sg, K = _seed_arrays(seeds, signs)
        out = np.empty(int(L_params), np.float32)
        self._check(_lib.flm_store_unmask_unpack_noise_f32(self.h, sd.ctypes.data_as(_u8p), sg.ctypes.data_as(_i8p), K,
                                                           int(L_params), int(frac_bits), float(clip), int(pack),
                                                           int(noise_bits), int(count), out.ctypes.data_as(_f32p)))
        return out

    def unmask_unpack_mod_f32(self, seeds, signs, L_params, frac_bits, clip, pack, count=1, noise_bits=0, guard=1):
        """unmask_unpack_f32 with the decode modulo the field (decode_unpack_mod; :538-540, :605): returns
        (float32[L_params], (near, max_abs)), the devices' near counts added and the maximum of their maxima."""
        sd, sg, K = _seed_arrays(seeds, signs)
        out, st = np.empty(int(L_params), np.float32), np.zeros(2, np.uint32)
        self._check(_lib.flm_store_unmask_unpack_mod_f32(self.h, sd.ctypes.data_as(_u8p), sg.ctypes.data_as(_i8p), K,
                                                         int(L_params), int(frac_bits), float(clip), int(pack),
                                                         int(noise_bits), int(count), int(guard),
                                                         out.ctypes.data_as(_f32p), st.ctypes.data_as(_u32p)))
        return out, (int(st[0]), int(st[1]))

    def reset(self):
        self._check(_lib.flm_store_reset(self.h))
