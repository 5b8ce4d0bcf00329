"""Simulation-wide protocol state shared by the Flamingo agents (the role util/param.py plays).

Holds the root seed, the vector length and the committee parameters, the one
GPU engine of this process, and caches the committee and the per-iteration
neighbour graph (the reference re-derives the graph in every findNeighbors
call, util/param.py:56-103; here it is derived once per iteration for all
clients, with the keystream computed on the GPU).

The simulation's P-256 work is batched across clients, because one scalar
multiplication is a ~3 ms latency chain on the GPU whatever the batch size
(DESIGN.md section 5): every ECDH point a_i A_j of the iteration's graph and
of the client x committee pairs (symmetric, so one per unordered pair), and
every client's ElGamal r G, r pk of the iteration, are computed in one launch
each and handed to the agents.  The values are those each client would
compute alone (SA_ClientAgent.py:234-236, 256-263, 434-447).
"""
from __future__ import annotations

import os

from ... import params as P

root_seed: bytes = os.urandom(32)     # util/param.py:31 draws it at import time too
vector_len: int = P.vector_len       # util/param.py:8
vector_type = P.vector_type
committee_size: int = P.committee_size
fraction: float = P.fraction
nonce = P.nonce

_engine = None
_group = None
_graphs: dict = {}
_committees: dict = {}
_pkis: dict = {}
_h2c: dict = {}           # h_ijt -> point, memoised lookups of the GPU table
_h2c_table = None         # (out (65536, 64), flags): hash_str_to_curve(str(v)) for every v < 2^16
_ecdh: dict = {}          # (root, N, min(i,j), max(i,j)) -> 64-byte wire of a_i A_j
_ecdh_done: set = set()   # batches already computed (graph iterations, committee)
_clients: dict = {}       # id -> client agent (for the batched ElGamal draws)
_elgamal: dict = {}       # (root, iteration, id) -> (r list, (deg, 64) rG wire, (deg, 64) c1 = H + r pk wire)
_pair_keys: dict = {}     # (root, N, min(i,j), max(i,j)) -> r_ij = SHA-256(a_i A_j)[:32] (symmetric)
_pair_mat: dict = {}      # (root, iteration, N, nsize) -> {id: PairMaterial}
# The clients' m_i shares are dealt and sealed for the whole iteration in two GPU launches
# (mi_shares); False takes the host path per client (seeds.shamir_share, crypto.aes_gcm_*), which
# sends byte-identical messages: the A/B switch of tools/deal_bench.py and tests/test_deal_gpu.py.
_gpu_deal: bool = True    # configure(gpu_deal=...)
_mi_draws: dict = {}      # (root, iteration, id) -> (m_i bytes, T-1 coefficients, C nonces)
_mi_shares: dict = {}     # (root, iteration, id) -> [(ciphertext, nonce)] in committee order
# The committee's check of the signatures the server forwards in DEC (the reference's
# `# CHECK SIGNATURES`, SA_ClientAgent.py:387): off by default, so a run sends what it always sent.
_check_signatures: bool = False        # configure(check_signatures=...)
# The sealed m_i shares keep their AES-GCM tag (the reference drops it, SA_ClientAgent.py:242, and
# opens without verify, :423-425): off by default, so a run sends what it always sent.
_authenticate_shares: bool = False     # configure(authenticate_shares=...)
# A member's 61 rows take as long in one GPU call as in the host loop (one wave's 2.6 ms chain against
# 61 x 43 us of OpenSSL), so the members verify on the host unless told otherwise.
_gpu_verify: bool = False              # configure(gpu_verify=True): one MaskEngine.ecdsa_verify call per DEC
_signature_quorum = 2 / 3               # configure(signature_quorum=...): the share of the committee whose
                                        # signatures over the same labels must verify
# The committee generates the system key itself (config_flamingo's --dkg: a joint-Feldman DKG among the
# members, abides/dkg) instead of receiving Shamir shares of a key the server knows (the reference's
# set-up, SA_ServiceAgent.py:261-279): off by default, so a run sends what it always sent.
_dkg: bool = False                      # configure(dkg=...)
_dkg_result = None                      # (group key, {committee member id: (member index, key share)})
# Float inputs (config_flamingo's --float_inputs F,CLIP[,sr]): a client's input_vector is float32 and goes through
# the fixed-point codec fused into its masking (MaskEngine.client_encode_mask); the server keeps final_sum and
# adds final_mean.  Off by default, so a run sends what it always sent and draws what it always drew.
_codec = None                           # configure(codec=(frac_bits, clip, "nearest" | "stochastic"))
# ... and, with a fourth element 2 or 4, that many parameters per ring word (the packed codec): a VECTOR body,
# the store, the masks and the sums are ring_len() = ceil(vector_len / pack) words; vector_len stays the
# parameter count and final_mean's length
_codec_pack: int = 1
# Distributed differential privacy (config_flamingo's --dp_noise BITS): every client adds a share of binomial
# noise, BITS fair coins per parameter, to its quantised update inside the masking kernel
# (MaskEngine.client_encode_noise_mask); only the sum of the shares appears in what the server unmasks.  It needs
# the float inputs.  Off by default, so a run sends what it always sent and draws what it always drew.
_dp_noise: int = 0
# ... or of discrete Gaussian noise (config_flamingo's --dp_gauss SIGMA[,TAIL]): the share is sampled from a cumulative
# table of the discrete Gaussian of parameter SIGMA truncated to +-TAIL (flamingo_amd.dgauss.table, built once here),
# inside the same kernel (MaskEngine.client_encode_gauss_mask); rows decode as binomial rows of 2 TAIL coins do.  It
# needs the float inputs and excludes --dp_noise.  Off (None) by default, so a run calls what it always called, sends
# what it always sent and draws what it always drew.
_dp_gauss: tuple | None = None          # (sigma, tail)
_dp_gauss_table = None                  # the (2 tail,) uint64 table of _dp_gauss
# Randomised block Hadamard rotation (config_flamingo's --rotate LOG2BLOCK): every client rotates its float update
# in blocks of 2^LOG2BLOCK parameters under the iteration's public key before the encode (MaskEngine.rotate), the
# server rotates the decoded mean back; the clip then bounds rotated coordinates.  It needs the float inputs.  Off
# by default, so a run sends what it always sent and draws what it always drew.
_rotate: int = 0
# L2 clip (config_flamingo's --l2_clip C): every client scales its float update to an L2 norm of at most C before the
# rotation, or with it when the rotation is on (MaskEngine.l2_clip, MaskEngine.rotate(clip_norm=...)), so that one
# client moves the sum by at most C in L2.  It needs the float inputs.  Off (None) by default, so a run calls what it
# always called, sends what it always sent and draws what it always drew.
_l2_clip: float | None = None
# Conditional stochastic rounding (config_flamingo's --round_bound TAIL[,ATTEMPTS]): every client draws ATTEMPTS
# candidate dither seeds where it draws one today and encodes with the first whose rounded row has a sum of squares
# within round_max_sumsq() (MaskEngine.round_select), so that Delta / 2^f bounds the L2 norm of what one client adds
# to the ring.  It needs stochastic float inputs and the L2 clip.  Off (None) by default, so a run calls what it
# always called, sends what it always sent and draws what it always drew.
_round_bound: tuple | None = None      # (tail k, attempts)
# Decode modulo the field (config_flamingo's --modular FRACTION): the server admits the cohort by
# MaskEngine.codec_check_modular (one contributor's field fits; n times the bias is not bounded) where it applies the
# worst-case headroom rule, decodes the packed sum with the carry-aware decode (MaskEngine.decode_unpack_mod,
# VectorStore.unmask_unpack_mod_f32) and keeps the near-wrap evidence at the guard ceil(FRACTION H).  It needs packed float
# inputs; the clients are unchanged.  Off (None) by default, so a run calls what it always called and refuses what it
# always refused.
_modular: float | None = None          # the guard's fraction of H, in (0, 1]
ROUND_BATCHES = 8                       # batches of candidates a client draws before it gives up


def configure(root: bytes | None = None, L: int | None = None, committee: int | None = None,
              gpu_deal: bool | None = None, check_signatures: bool | None = None,
              signature_quorum: float | None = None, gpu_verify: bool | None = None,
              authenticate_shares: bool | None = None, dkg: bool | None = None, codec=None,
              dp_noise: int | None = None, rotate: int | None = None, l2_clip: float | None = None, round_bound=None,
              dp_gauss=None, modular=None):
    """Reset the protocol parameters (between simulations / in tests).  codec: (frac_bits, clip, "nearest" or
    "stochastic") turns the float inputs on, (frac_bits, clip, rounding, pack) with pack 1, 2 or 4 also packs that
    many parameters into a ring word, False turns them off, None leaves them as they are.  dp_noise: the coin
    flips per parameter of every client's binomial noise share (even, 2..1024; 0 turns it off, None leaves it as
    it is); it needs the float inputs, and turning those off turns it off.  rotate: log2 of the block of the randomised
    Hadamard rotation in front of the codec (4..12; 0 turns it off, None leaves it as it is); it needs the float
    inputs, and turning those off turns it off.  l2_clip: the L2 norm every client scales its update down to (finite
    and positive; 0 turns it off, None leaves it as it is); it needs the float inputs, and turning those off turns it
    off.  round_bound: (tail, attempts) or a bare tail (attempts = 4) turns conditional stochastic rounding on: tail =
    k >= 0 of the bound, attempts in 1..8 candidate dither seeds per batch; 0 or False turns it off, None leaves it as
    it is; it needs stochastic float inputs and the L2 clip, and turning either off turns it off.  dp_gauss: (sigma,
    tail) or a bare sigma (tail = ceil(10 sigma)) turns the discrete Gaussian noise share on, tail in 1..512; 0 or False
    turns it off, None leaves it as it is; it needs the float inputs (turning those off turns it off) and is refused
    together with dp_noise.  modular: a fraction in (0, 1] turns the decode modulo the field on, with the guard
    ceil(fraction H) of its near-wrap count; 0 or False turns it off, None leaves it as it is; it needs a packed codec
    (pack 2 or 4), and turning the float inputs off turns it off."""
    global root_seed, vector_len, committee_size, _h2c_table, _gpu_deal, _check_signatures, _signature_quorum, _gpu_verify
    global _authenticate_shares, _dkg, _dkg_result, _codec, _codec_pack, _dp_noise, _rotate, _l2_clip, _round_bound
    global _dp_gauss, _dp_gauss_table, _modular
    if codec is not None:
        if codec is False:
            _codec, _codec_pack, _dp_noise, _rotate, _l2_clip, _round_bound = None, 1, 0, 0, None, None
            _dp_gauss, _dp_gauss_table, _modular = None, None, None
        else:
            f, c, mode = codec[:3]
            pack = int(codec[3]) if len(codec) == 4 else 1
            if len(codec) not in (3, 4):
                raise ValueError("codec is (frac_bits, clip, rounding) or (frac_bits, clip, rounding, pack)")
            if mode not in ("nearest", "stochastic"):
                raise ValueError("codec rounding must be 'nearest' or 'stochastic'")
            if pack not in (1, 2, 4):
                raise ValueError("codec pack must be 1, 2 or 4")
            _codec, _codec_pack = (int(f), float(c), mode), pack
    gauss_off = dp_gauss is False or (dp_gauss is not None and not isinstance(dp_gauss, (tuple, list)) and float(dp_gauss) == 0.0)
    if dp_noise is not None:
        b = int(dp_noise)
        if b < 0 or b > 1024 or b % 2:
            raise ValueError("dp_noise must be even and in 0..1024")
        if b and _codec is None:
            raise ValueError("dp_noise needs the float inputs (codec=...)")
        if b and not gauss_off and (dp_gauss is not None or _dp_gauss is not None):
            raise ValueError("dp_noise and dp_gauss exclude each other")
        _dp_noise = b
    if dp_gauss is not None:
        if gauss_off:
            _dp_gauss, _dp_gauss_table = None, None
        else:
            from ... import dgauss
            sigma = float(dp_gauss[0] if isinstance(dp_gauss, (tuple, list)) else dp_gauss)
            tail = dp_gauss[1] if isinstance(dp_gauss, (tuple, list)) and len(dp_gauss) > 1 and dp_gauss[1] is not None \
                else dgauss.default_tail(sigma) if sigma > 0.0 else 0
            if _codec is None:
                raise ValueError("dp_gauss needs the float inputs (codec=...)")
            if _dp_noise:
                raise ValueError("dp_noise and dp_gauss exclude each other")
            if int(tail) != tail or not 1 <= int(tail) <= dgauss.MAX_TAIL:
                raise ValueError(f"dp_gauss's tail must be an integer in 1..{dgauss.MAX_TAIL} (the default is ceil(10 sigma))")
            table = dgauss.table(sigma, int(tail))      # refuses a sigma that is not finite and positive
            _dp_gauss, _dp_gauss_table = (sigma, int(tail)), table
    if rotate is not None:
        h = int(rotate)
        if h != 0 and not 4 <= h <= 12:
            raise ValueError("rotate must be 0 or a log2 block size in 4..12")
        if h and _codec is None:
            raise ValueError("rotate needs the float inputs (codec=...)")
        _rotate = h
    if l2_clip is not None:
        import ctypes
        import math
        c = ctypes.c_float(float(l2_clip)).value   # the float32 radius the library takes
        if l2_clip != 0 and not (math.isfinite(c) and c > 0.0):
            raise ValueError("l2_clip must be 0 or a finite positive norm")
        if c and _codec is None:
            raise ValueError("l2_clip needs the float inputs (codec=...)")
        _l2_clip = c if c else None
    if round_bound is not None:
        import math
        if round_bound is False or (not isinstance(round_bound, (tuple, list)) and float(round_bound) == 0.0):
            _round_bound = None
        else:
            tail, attempts = round_bound if isinstance(round_bound, (tuple, list)) else (round_bound, 4)
            tail = float(tail)
            if not (math.isfinite(tail) and tail >= 0.0):
                raise ValueError("round_bound's tail must be finite and not negative")
            if int(attempts) != attempts or not 1 <= int(attempts) <= 8:
                raise ValueError("round_bound's attempts must be in 1..8")
            if _codec is None or _codec[2] != "stochastic":
                raise ValueError("round_bound needs stochastic float inputs (codec=(f, clip, 'stochastic'))")
            if _l2_clip is None:
                raise ValueError("round_bound needs the L2 clip (l2_clip=...)")
            _round_bound = (tail, int(attempts))
    if _round_bound is not None and (_codec is None or _codec[2] != "stochastic" or _l2_clip is None):
        _round_bound = None                   # what it stands on was turned off
    if modular is not None:
        import math
        if modular is False or float(modular) == 0.0:
            _modular = None
        else:
            fr = float(modular)
            if not (math.isfinite(fr) and 0.0 < fr <= 1.0):
                raise ValueError("modular must be a fraction in (0, 1] (0 turns it off)")
            if _codec is None or _codec_pack not in (2, 4):
                raise ValueError("modular needs a packed codec (codec=(f, clip, rounding, 2 or 4))")
            _modular = fr
    if _modular is not None and (_codec is None or _codec_pack not in (2, 4)):
        raise ValueError("modular needs a packed codec (codec=(f, clip, rounding, 2 or 4))")
    if dkg is not None:
        _dkg = bool(dkg)
    _dkg_result = None
    if authenticate_shares is not None:
        _authenticate_shares = bool(authenticate_shares)
    if gpu_deal is not None:
        _gpu_deal = bool(gpu_deal)
    if check_signatures is not None:
        _check_signatures = bool(check_signatures)
    if gpu_verify is not None:
        _gpu_verify = bool(gpu_verify)
    if signature_quorum is not None:
        if not 0 < float(signature_quorum) <= 1:
            raise ValueError("signature_quorum must be in (0, 1]")
        _signature_quorum = float(signature_quorum)
    _mi_draws.clear()
    _mi_shares.clear()
    if root is not None:
        if len(root) != 32:
            raise ValueError("root seed must be 32 bytes")
        root_seed = root
    if L is not None:
        vector_len = int(L)
    if committee is not None:
        committee_size = int(committee)
    _graphs.clear()
    _committees.clear()
    _pkis.clear()
    _ecdh.clear()
    _ecdh_done.clear()
    _clients.clear()
    _elgamal.clear()
    _pair_keys.clear()
    _pair_mat.clear()
    _h2c.clear()                 # the table is the engine's: recomputed with whatever engine is current
    _h2c_table = None


def shutdown():
    """Close the server's device group (its RCCL clique included) and the process engine, after the
    stores on them are closed; the next engine()/server_engine() call starts afresh."""
    global _engine, _group
    configure()
    if _group is not None:
        _group.close()
        _group = None
    if _engine is not None:
        _engine.close()
        _engine = None


def engine():
    """The process's MaskEngine (created lazily: after any fork, before first use)."""
    global _engine
    if _engine is None:
        from ...engine import MaskEngine
        _engine = MaskEngine(int(os.environ.get("FLM_DEVICE", "0")))
    return _engine


def server_devices() -> list:
    """Devices the server's vector steps use: FLM_GROUP_DEVICES ("0,1,2,..."; one id repeated =
    loopback ranks on one GPU), else FLM_GPUS devices 0..n-1 (FLM_GPUS=all: every visible GPU),
    else the process's one device (FLM_DEVICE).  A multi-GPU group is opt-in."""
    spec = os.environ.get("FLM_GROUP_DEVICES", "").strip()
    if spec:
        return [int(d) for d in spec.split(",")]
    n = os.environ.get("FLM_GPUS", "").strip().lower()
    if n == "all":
        from ... import _lib
        return list(range(max(1, int(_lib.load().flm_device_count()))))
    if n and int(n) > 1:
        return list(range(int(n)))
    return [int(os.environ.get("FLM_DEVICE", "0"))]


def server_group_rccl() -> bool:
    """FLM_GROUP_RCCL=1: a one-device server group still gets an RCCL clique (flm_group_init_flags
    with FLM_GROUP_RCCL), so the drop-in server runs the multi-GPU code path on one GPU."""
    return os.environ.get("FLM_GROUP_RCCL", "").strip() not in ("", "0")


def server_engine():
    """The server's partial sum and unmask (SA_ServiceAgent.py:346-350, 529-605) run on every
    device of server_devices(): a DeviceGroup (client-sharded rows, slot-sharded masks, one RCCL
    reduce-scatter) when that is more than one (or FLM_GROUP_RCCL asks for a one-device clique),
    else the process MaskEngine.  Should the group not come up (RCCL missing, a device refused),
    the server says so and stays on one GPU.  The group is kept while the device list and the
    requested FLM_GROUP_RCCL flag stay the same (a group of distinct devices always has a clique,
    so it is the request that is compared, not flm_group_has_rccl).  A group replaced while a
    VectorStore still uses it is marked retired and closed by that store's close() (the agent swaps
    its store at the next iteration boundary, SA_ServiceAgent.reconstruction_clear_pool)."""
    global _group
    devs = server_devices()
    force = server_group_rccl()
    if len(devs) == 1 and devs[0] == int(os.environ.get("FLM_DEVICE", "0")) and not force:
        return engine()
    if _group is None or _group.devices != devs or _group.force_rccl != force:
        from ...engine import DeviceGroup
        if _group is not None:
            if _group._stores:
                _group.retired = True      # closed by its last VectorStore's close()
            else:
                _group.close()
            _group = None
        try:
            _group = DeviceGroup(devs, force_rccl=force)
        except RuntimeError as e:
            import warnings
            warnings.warn(f"server device group {devs} unavailable ({e}); using one GPU")
            return engine()
    return _group


def vector_store(L: int, capacity: int):
    """The server's device-resident VECTOR store (flamingo_amd.ingest.VectorStore) on
    server_engine()'s device(s).  An engine object that brings its own store (a test double)
    provides it through a `vector_store(L, capacity)` method."""
    eng = server_engine()
    own = getattr(eng, "vector_store", None)
    if own is not None:
        return own(L, capacity)
    from ...ingest import VectorStore
    return VectorStore(eng, L, capacity)


def committee(num_clients: int) -> set:
    key = (root_seed, committee_size, num_clients)
    if key not in _committees:
        _committees[key] = P.choose_committee(root_seed, committee_size, num_clients,
                                              encrypt=engine().chacha20_encrypt)
    return _committees[key]


def neighbors(iteration: int, num_clients: int, neighborhood_size: int) -> list:
    key = (root_seed, iteration, num_clients, neighborhood_size)
    if key not in _graphs:
        _graphs.clear() if len(_graphs) > 8 else None
        _graphs[key] = P.neighbor_graph(root_seed, iteration, num_clients, neighborhood_size,
                                        encrypt=engine().chacha20_encrypt)
    return _graphs[key]


def find_neighbors(root, current_iteration, num_clients, id, neighborhood_size) -> set:
    """util/param.findNeighbors signature."""
    if root != root_seed:
        return P.find_neighbors(root, current_iteration, num_clients, id, neighborhood_size,
                                encrypt=engine().chacha20_encrypt)
    return neighbors(current_iteration, num_clients, neighborhood_size)[id]


def pki(num_clients: int):
    """Key material for this simulation (pki_files/ stand-in, see pki.py).  With configure(dkg=True)
    the system key is the committee's (set_dkg_result must have run): its public half is the DKG's
    group key and nobody holds the private half."""
    key = (root_seed, num_clients)
    if key not in _pkis:
        from .pki import PKI
        _pkis.clear()
        if _dkg and _dkg_result is None:
            raise RuntimeError("configure(dkg=True): the committee's key generation has not run (set_dkg_result)")
        _pkis[key] = PKI(root_seed, num_clients, engine(), system_pk=_dkg_result[0] if _dkg else None)
    return _pkis[key]


def codec():
    """(frac_bits, clip, rounding) of the float inputs, or None when they are off (configure(codec=...))."""
    return _codec


def codec_pack() -> int:
    """Parameters per ring word of the float inputs: 1 (also when they are off), 2 or 4."""
    return _codec_pack if _codec is not None else 1


def codec_noise_bits() -> int:
    """Coin flips per parameter of every client's binomial noise share: 0 when off (or the float inputs are)."""
    return _dp_noise if _codec is not None else 0


def dp_gauss() -> tuple | None:
    """(sigma, tail) of the clients' discrete Gaussian noise share, or None when it is off."""
    return _dp_gauss if _codec is not None else None


def dp_gauss_table():
    """The cumulative table of dp_gauss() (2 tail uint64 entries, built once by configure), or None."""
    return _dp_gauss_table if _codec is not None else None


def decode_noise_bits() -> int:
    """What the packed decode and the headroom rule take for noise_bits: the binomial share's coins, or 2 tail of the
    discrete Gaussian one (the same bias B + tail); 0 without noise."""
    return 2 * _dp_gauss[1] if dp_gauss() is not None else codec_noise_bits()


def modular() -> float | None:
    """The guard's fraction of H of the decode modulo the field, or None when it is off (or the float inputs are)."""
    return _modular if _codec is not None else None


def modular_guard() -> int:
    """The integer guard of the decode modulo the field: flamingo_amd.modular.guard(pack, fraction)."""
    from ...modular import guard
    return guard(_codec_pack, _modular)


def rotate_bits() -> int:
    """log2 of the rotation's block: 0 when the rotation is off (or the float inputs are)."""
    return _rotate if _codec is not None else 0


def l2_clip() -> float | None:
    """The L2 norm the clients scale their updates down to, or None when that is off (or the float inputs are)."""
    return _l2_clip if _codec is not None else None


def round_bound() -> tuple | None:
    """(tail, attempts) of conditional stochastic rounding, or None when it is off."""
    return _round_bound if _codec is not None else None


def round_max_sumsq() -> int:
    """Delta^2, the bound on the sum of squares of a client's rounded row: MaskEngine.round_bound of the L2 clip, the
    codec's frac_bits, the coordinates encoded (rotated_len()) and the tail.  The server and every client compute it
    with this one call, so they agree."""
    return engine().round_bound(_l2_clip, _codec[0], rotated_len(), tail=_round_bound[0])


def rotated_len() -> int:
    """Parameters the codec sees: vector_len, rounded up to whole blocks of the rotation when it is on."""
    H = 1 << rotate_bits()
    return -(-vector_len // H) * H


def rotation_key(iteration: int) -> bytes:
    """The iteration's public rotation key, the same for every client and the server:
    SHA-256(b"flamingo rotation" || root_seed || iteration as 8 bytes little-endian)."""
    import hashlib
    return hashlib.sha256(b"flamingo rotation" + root_seed + int(iteration).to_bytes(8, "little")).digest()


def ring_len() -> int:
    """Words of a ring row (a VECTOR body, a mask, the sums): ceil(rotated_len() / codec_pack())."""
    return -(-rotated_len() // codec_pack())


def dkg_on() -> bool:
    """True when the committee's key comes from its own key generation (configure(dkg=True))."""
    return _dkg


def set_dkg_result(group_key, shares: dict) -> None:
    """The outcome of the committee's key generation: the group key and, per committee member id,
    (member index, key share) -- what COMMITTEE_SHARED_SK carries in the default set-up."""
    global _dkg_result
    if group_key is None:
        raise RuntimeError("the key generation ended with the group key at infinity")
    _dkg_result = (group_key, dict(shares))
    _pkis.clear()


def dkg_share(member_id: int):
    """(member index, key share) of a committee member from the key generation, None for others."""
    return _dkg_result[1].get(member_id) if _dkg_result is not None else None


def hash_to_curve(h_ijt: str):
    """ecchash.hash_str_to_curve(h_ijt, 2, n, m, L, XMD-SHA256) as the client calls it
    (SA_ClientAgent.py:283-286), on the GPU.  h_ijt is str(x & 0xFFFF) (:280), so the first call
    computes the whole table of the 2^16 possible points in one launch
    (MaskEngine.hash_to_curve_decimal) and every later call is a lookup; any other message is
    hashed by its own launch.  Returns the affine point (x, y), or None for infinity."""
    pt = _h2c.get(h_ijt)
    if pt is not None:
        return pt
    if h_ijt.isdigit() and str(int(h_ijt)) == h_ijt and int(h_ijt) < (1 << 16):
        out, fl = h2c_table()
        row, f = out[int(h_ijt)], int(fl[int(h_ijt)])
    else:
        out, fl = engine().hash_to_curve_wire([h_ijt])
        row, f = out[0], int(fl[0])
    b = row.tobytes()
    pt = _h2c[h_ijt] = None if f & 4 else (int.from_bytes(b[:32], "big"), int.from_bytes(b[32:], "big"))
    return pt


# ------------------------------------------------------- batched P-256 work
def _ecdh_batch(num_clients: int, pairs) -> None:
    """a_i A_j for every (i, j) in pairs not cached yet, in one GPU launch.  i == j is kept: a
    committee member that is also a client encrypts its own m_i share under a_i A_i (:234-236)."""
    from ... import crypto as C
    import numpy as np
    kp = pki(num_clients)
    todo = sorted({(min(i, j), max(i, j)) for i, j in pairs} -
                  {k[2:] for k in _ecdh if k[:2] == (root_seed, num_clients)})
    if not todo:
        return
    a = [kp.client_sk[i] for i, _ in todo]
    out, _ = engine().ec_mul_wire(kp.pk_wire([j for _, j in todo]), C.scalars_to_wire(a))
    for (i, j), row in zip(todo, np.asarray(out)):
        _ecdh[(root_seed, num_clients, i, j)] = bytes(row)


def prefetch_graph_ecdh(iteration: int, num_clients: int, neighborhood_size: int) -> None:
    key = ("graph", root_seed, iteration, num_clients, neighborhood_size)
    if key in _ecdh_done:
        return
    nb = neighbors(iteration, num_clients, neighborhood_size)
    _ecdh_batch(num_clients, [(i, j) for i in range(num_clients) for j in nb[i]])
    _ecdh_done.add(key)


def prefetch_committee_ecdh(num_clients: int) -> None:
    key = ("committee", root_seed, num_clients, committee_size)
    if key in _ecdh_done:
        return
    comm = sorted(committee(num_clients))
    _ecdh_batch(num_clients, [(i, c) for i in range(num_clients) for c in comm])
    _ecdh_done.add(key)


def ecdh_wire(num_clients: int, i: int, j: int) -> bytes:
    """a_i A_j (= a_j A_i) as 64 wire bytes x||y; computed in a batch if not prefetched."""
    k = (root_seed, num_clients, min(i, j), max(i, j))
    if k not in _ecdh:
        _ecdh_batch(num_clients, [(i, j)])
    return _ecdh[k]


def h2c_table():
    """(out (65536, 64), flags) of hash_str_to_curve(str(v)) for every v < 2^16, one GPU launch
    (computed on first use, kept for the simulation)."""
    global _h2c_table
    if _h2c_table is None:
        _h2c_table = engine().hash_to_curve_decimal(0, 1 << 16)
    return _h2c_table


def pair_material(iteration: int, num_clients: int, neighborhood_size: int) -> dict:
    """Every client's pairwise seeds of `iteration` in a few batched launches
    (SA_ClientAgent.py:253-292): id -> (nb, h, H, s) with nb the neighbour list in the reference's
    set order, h the h_ijt strings, H the (deg, 64) wire rows of hash_str_to_curve(h_ijt) and s the
    32-byte seeds SHA-256(H).  r_ij = SHA-256(a_i A_j) comes from the graph's ECDH batch; every h_ijt
    of the iteration from ONE PRG launch (client_agent.pair_prf); H from the hash-to-curve table."""
    import hashlib
    import numpy as np
    key = (root_seed, iteration, num_clients, neighborhood_size)
    if key in _pair_mat:
        return _pair_mat[key]
    from .client_agent import pair_prf
    nbrs = neighbors(iteration, num_clients, neighborhood_size)
    prefetch_graph_ecdh(iteration, num_clients, neighborhood_size)
    lists = [list(nbrs[i]) for i in range(num_clients)]
    keys = []
    for i, nb in enumerate(lists):
        for j in nb:
            k = (root_seed, num_clients, min(i, j), max(i, j))
            r = _pair_keys.get(k)
            if r is None:
                r = _pair_keys[k] = hashlib.sha256(ecdh_wire(num_clients, i, j)).digest()[:32]
            keys.append(r)
    hs = pair_prf(engine(), keys, iteration)
    out, fl = h2c_table()
    rows = [np.asarray(out[int(h)], np.uint8) for h in hs]
    mat, o = {}, 0
    for i, nb in enumerate(lists):
        n = len(nb)
        H = np.stack(rows[o:o + n]) if n else np.zeros((0, 64), np.uint8)
        if n and any(int(fl[int(h)]) & 4 for h in hs[o:o + n]):
            raise RuntimeError("hash_to_curve gave the point at infinity")      # not in the 2^16 table
        mat[i] = (nb, hs[o:o + n], H, [hashlib.sha256(r.tobytes()).digest() for r in H])
        o += n
    for k in [k for k in _pair_mat if k[1] < iteration - 1]:
        del _pair_mat[k]
    _pair_mat[key] = mat
    return mat


def register_client(agent) -> None:
    _clients[agent.id] = agent


def elgamal_masks(agent, iteration: int, nb: list):
    """(r list, c0 = r G wire rows, c1 = H + r pk_system wire rows) for this client's neighbours in
    `iteration` (SA_ClientAgent.py:326-332, 434-447), H the pair's hash-to-curve point
    (pair_material).  The first client to ask in an iteration draws every registered, online
    client's r's from that client's own random state and computes all of them in two launches:
    r G and r pk (flm_ec_mul), then H + r pk (flm_ec_combine with one term of coefficient 1)."""
    from ... import crypto as C
    import numpy as np
    key = (root_seed, iteration, agent.id)
    if key not in _elgamal:
        batch = []
        for cid in sorted(_clients):
            c = _clients[cid]
            if iteration in c.offline_iterations or (root_seed, iteration, cid) in _elgamal:
                continue
            cnb = list(neighbors(iteration, c.num_clients, c.neighborhood_size)[cid])
            batch.append((cid, [c._rand_scalar() for _ in cnb]))
        if agent.id not in [b[0] for b in batch]:
            batch.append((agent.id, [agent._rand_scalar() for _ in nb]))
        rs = [r for _, r_list in batch for r in r_list]
        if rs:
            sys_pk = pki(agent.num_clients).system_pk
            base = np.concatenate([np.tile(np.frombuffer(C.point_bytes(C.G), np.uint8), (len(rs), 1)),
                                   np.tile(np.frombuffer(C.point_bytes(sys_pk), np.uint8), (len(rs), 1))])
            out, _ = engine().ec_mul_wire(base, C.scalars_to_wire(rs + rs))
            out = np.asarray(out)
            pm = pair_material(iteration, agent.num_clients, agent.neighborhood_size)
            H = np.concatenate([pm[cid][2] for cid, r_list in batch if r_list])
            c1, _, fl = engine().ec_combine_wire(H, out[len(rs):][None], C.scalars_to_wire([1]), negate=False)
            c1 = np.asarray(c1)
            if (np.asarray(fl) & 4).any():
                raise RuntimeError("ElGamal c1 = H + r pk at infinity")
        o = 0
        for cid, r_list in batch:
            n = len(r_list)
            _elgamal[(root_seed, iteration, cid)] = (r_list, out[o:o + n] if n else None, c1[o:o + n] if n else None)
            o += n
        for k in [k for k in _elgamal if k[1] < iteration - 1]:
            del _elgamal[k]
    return _elgamal.pop(key)


# ------------------------------------------------ m_i shares: dealt and sealed in one batch
def deal_on_gpu() -> bool:
    """True when the clients' m_i shares go through mi_shares (configure(gpu_deal=True), the
    default).  An engine object that brings no dealing calls (a CPU test double, as for
    vector_store) leaves the agents on the host path, which sends the same bytes."""
    calls = ("shamir_deal_wire", "aes_gcm_xor_wire") + (("aes_gcm_seal_wire", "aes_gcm_open_wire")
                                                       if _authenticate_shares else ())
    return _gpu_deal and all(hasattr(engine(), c) for c in calls)


# ------------------------------------------------ authenticated sealing of the m_i shares
SHARE_TAG_LEN = 16


def authenticate_shares_on() -> bool:
    """True when the m_i shares travel with their AES-GCM tag and the committee verifies it
    (configure(authenticate_shares=True); off by default)."""
    return _authenticate_shares


def share_aad(iteration: int, dealer: int, member: int) -> bytes:
    """What a sealed share is bound to besides its key: iteration (8 bytes) || dealer id (4) ||
    committee member id (4), big endian.  The pair key is a static ECDH key, so without the
    iteration last iteration's ciphertext of the same dealer would still verify."""
    return int(iteration).to_bytes(8, "big") + int(dealer).to_bytes(4, "big") + int(member).to_bytes(4, "big")


# ------------------------------------------------ the committee's signature check
def check_signatures_on() -> bool:
    """True when a committee member verifies the signatures of a DEC before it releases its
    decryption shares (configure(check_signatures=True); off by default)."""
    return _check_signatures


def signatures_needed(committee_members: int) -> int:
    """ceil(signature_quorum x committee size): how many members' signatures over the labels a
    member signed itself must verify before it goes on."""
    from fractions import Fraction
    import math
    return max(1, math.ceil(Fraction(_signature_quorum).limit_denominator(1 << 20) * committee_members))


def verify_signatures(pubs, msgs, sigs) -> list:
    """One verdict per (public key, message, signature) row: crypto.ecdsa_verify row by row (the
    default: at a member's 61 rows the GPU call is no faster), or after configure(gpu_verify=True)
    the engine's batched GPU call (MaskEngine.ecdsa_verify, one launch for the whole DEC) where the
    engine has it (a CPU test double does not)."""
    from ... import crypto as C
    batch = getattr(engine(), "ecdsa_verify", None) if _gpu_verify else None
    if batch is not None:
        return [bool(v) for v in batch(pubs, msgs, sigs)]
    return [pub is not None and len(sig) == 64 and C.ecdsa_verify(pub, msg, sig)
            for pub, msg, sig in zip(pubs, msgs, sigs)]


def check_dec_signatures(num_clients: int, server_labels, dec_labels, own_payload) -> tuple:
    """What a committee member checks when DEC arrives (SA_ClientAgent.py:387, the server's side at
    SA_ServiceAgent.py:382-386).  server_labels: the (labels, signature) pair of the SIGN message it
    stored; dec_labels: sender -> (payload, signature) as forwarded; own_payload: what this member
    signed.  All rows -- the server's signature under pki.server_pk, every entry under its sender's
    key -- go through ONE verify_signatures call.  An entry counts when its signature verifies, its
    sender sits on the committee and its payload is the member's own.
    Returns (server_ok, count, needed)."""
    keys = pki(num_clients)
    members = committee(num_clients)
    entries = []
    for sender, signed in (dec_labels or {}).items():
        if (isinstance(sender, int) and 0 <= sender < num_clients and isinstance(signed, (tuple, list))
                and len(signed) == 2 and all(isinstance(b, (bytes, bytearray)) for b in signed)):
            entries.append((sender, bytes(signed[0]), bytes(signed[1])))
    try:
        labels, server_sig = bytes(server_labels[0]), bytes(server_labels[1])
    except (TypeError, IndexError, ValueError):
        labels, server_sig = b"", b""
    verdicts = verify_signatures([keys.server_pk] + [keys.client_pk[s] for s, _, _ in entries],
                                 [labels] + [p for _, p, _ in entries], [server_sig] + [g for _, _, g in entries])
    count = sum(1 for ok, (sender, payload, _) in zip(verdicts[1:], entries)
                if ok and sender in members and payload == own_payload)
    return bool(verdicts[0]), count, signatures_needed(len(members))


def _mi_shape(agent) -> tuple:
    """(threshold T, committee size C) of the m_i dealing (SA_ClientAgent.py:216-220)."""
    C = len(agent.user_committee)
    return max(1, int(fraction * C)), C


def _draw_mi(agent) -> tuple:
    """m_i, the T - 1 polynomial coefficients and the C nonces from the client's own random state,
    in the reference's order (SA_ClientAgent.py:214-240): 32 bytes, 40 bytes mod n per coefficient
    (client_agent._PyRandom), 16 bytes per nonce.  RandomState.randint(0, 256, dtype=uint8) spends
    one 32-bit word of the stream per four bytes and keeps none between calls, so with every size a
    multiple of four ONE draw of all the bytes is the same stream as the 1 + (T - 1) + C separate
    draws of the host path (tests/test_deal_cpu.py holds the two against each other)."""
    import numpy as np
    from .seeds import P256_N
    T, C = _mi_shape(agent)
    kl, rs = agent.key_length, agent.random_state
    if kl % 4 == 0:
        buf = bytes(rs.randint(0, 256, size=kl + 40 * (T - 1) + 16 * C, dtype=np.uint8))
    else:
        buf = b"".join(bytes(rs.randint(0, 256, size=s, dtype=np.uint8)) for s in [kl] + [40] * (T - 1) + [16] * C)
    o = kl + 40 * (T - 1)
    return (buf[:kl], [int.from_bytes(buf[kl + 40 * j: kl + 40 * j + 40], "big") % P256_N for j in range(T - 1)],
            [buf[o + 16 * k: o + 16 * k + 16] for k in range(C)])


def mi_draw(agent, iteration: int) -> tuple:
    """(m_i bytes, coefficients, nonces) of this client in `iteration`: drawn here, where
    sendVectors reaches SA_ClientAgent.py:214, unless mi_shares' batch drew them for it already."""
    key = (root_seed, iteration, agent.id)
    if key not in _mi_draws:
        _mi_draws[key] = _draw_mi(agent)
    return _mi_draws[key]


def mi_shares(agent, iteration: int) -> list:
    """This client's enc_mi_shares [(ciphertext, nonce), ...] in committee order
    (SA_ClientAgent.py:218-244): the Shamir shares of m_i at x = 1..C, each AES-128-GCM encrypted
    (tag dropped) under the key shared with that member (client_agent._aes_keys).  The first
    client to ask in an iteration deals every registered, online client's shares in ONE
    flm_shamir_deal launch and seals them in ONE flm_aes_gcm_xor launch -- or, with
    configure(authenticate_shares=True), ONE flm_aes_gcm_seal launch, the 16-byte tag appended to
    each ciphertext; no draw is added, so the draw order below holds either way.

    Every client's random state sees the draws of the host path in the same order, so the VECTOR
    messages stay byte-identical: a client draws its own m_i, coefficients and nonces through
    mi_draw at the start of sendVectors, and calls this after elgamal_masks, which has by then
    drawn every client's ElGamal r's; the batch draws here for the clients that have not reached
    sendVectors yet (their r's come first on the host path too), and they pick those values up
    from mi_draw instead of drawing again."""
    import numpy as np
    key = (root_seed, iteration, agent.id)
    if key not in _mi_shares:
        batch = [c for cid, c in sorted(_clients.items())
                 if iteration not in c.offline_iterations and (root_seed, iteration, cid) not in _mi_shares]
        if agent.id not in [c.id for c in batch]:
            batch.append(agent)
        T, C = _mi_shape(agent)
        members = sorted(agent.user_committee)
        if any(c.key_length != 32 or _mi_shape(c) != (T, C) for c in batch):
            raise RuntimeError("m_i shares are dealt as 32-byte values over one committee")
        draws = [mi_draw(c, iteration) for c in batch]
        M = len(batch)
        coeffs = np.empty((T, M, 32), np.uint8)
        coeffs[0] = np.frombuffer(b"".join(d[0] for d in draws), np.uint8).reshape(M, 32)
        if T > 1:
            coeffs[1:] = np.frombuffer(b"".join(v.to_bytes(32, "big") for d in draws for v in d[1]),
                                       np.uint8).reshape(M, T - 1, 32).transpose(1, 0, 2)
        shares = engine().shamir_deal_wire(coeffs, np.arange(1, C + 1, dtype=np.uint32))      # (C, M, 32)
        for c in batch:
            if not c.committee_keys:
                c.committee_keys = c._aes_keys(members)
        keys = np.frombuffer(b"".join(c.committee_keys[m] for c in batch for m in members), np.uint8).reshape(M * C, 16)
        nonces = np.frombuffer(b"".join(n for d in draws for n in d[2]), np.uint8).reshape(M * C, 16)
        plain = np.ascontiguousarray(shares.transpose(1, 0, 2)).reshape(M * C, 32)
        if _authenticate_shares:       # ciphertext || tag per share, bound to (iteration, dealer, member)
            aad = np.frombuffer(b"".join(share_aad(iteration, c.id, m) for c in batch for m in members),
                                np.uint8).reshape(M * C, 16)
            ct = np.concatenate(engine().aes_gcm_seal_wire(keys, nonces, plain, aad=aad), axis=1)
        else:
            ct = engine().aes_gcm_xor_wire(keys, nonces, plain)
        w = ct.shape[1]
        for i, (c, d) in enumerate(zip(batch, draws)):
            b = ct[i * C:(i + 1) * C].tobytes()
            _mi_shares[(root_seed, iteration, c.id)] = [(b[w * k: w * k + w], d[2][k]) for k in range(C)]
        for cache in (_mi_shares, _mi_draws):
            for k in [k for k in cache if k[1] < iteration - 1]:
                del cache[k]
    return _mi_shares[key]
