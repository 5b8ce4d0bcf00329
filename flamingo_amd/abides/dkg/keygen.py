"""State shared by the DKG agents of one simulation: the batched dealing, the share checks and the
group key (the role flamingo/protocol.py plays for the Flamingo agents).

Joint-Feldman key generation among n members (agent/dkg/SA_ClientAgent.py, SA_ServiceAgent.py):
member i deals a random polynomial f_i of degree t, sends f_i(j) to member j and broadcasts the
commitments C_{i,k} = c_{i,k} G; member j checks f_i(j) G == sum_k j^k C_{i,k}, complains where that
fails, the dealer answers a complaint by broadcasting the share, and a broadcast share that fails
disqualifies the dealer.  Over the agreed set QUAL, member j's key share is sum_i f_i(j) mod n and
the group key sum_i C_{i,0}.

On the GPU (the default) every dealer's shares are ONE flm_shamir_deal launch and every dealer's
commitments ONE flm_ec_mul launch, made when the first dealer asks and cached per dealer; a member
checks all shares of SHARE_AND_COMMIT in ONE flm_feldman_verify launch and the broadcast shares of
FORWARD_SHARE in one more; the group key is one flm_ec_combine.  configure(gpu_dkg=False) takes the
host path instead (seeds.shamir_share, crypto.mul, crypto.feldman_verify, crypto.add): every dealer
draws from its own random state in the same order either way, so the messages are byte-identical.
"""
from __future__ import annotations

import numpy as np

from ... import crypto as C
from ..flamingo import protocol as param
from ..flamingo.seeds import P256_N, shamir_share

fraction: float = param.fraction

_gpu_dkg: bool = True     # configure(gpu_dkg=...)
_dealers: dict = {}       # id -> dealer agent (for the batched dealing)
_dealt: dict = {}         # (root, id) -> (shares {receiver: (x, y)}, commitments [point or None])

_GPU_CALLS = ("shamir_deal_wire", "ec_mul_wire", "feldman_verify_wire", "ec_combine_wire")


def configure(gpu_dkg: bool | None = None):
    """Reset the DKG state (between simulations / in tests); gpu_dkg=False: the host path."""
    global _gpu_dkg
    if gpu_dkg is not None:
        _gpu_dkg = bool(gpu_dkg)
    _dealers.clear()
    _dealt.clear()


def on_gpu() -> bool:
    """True when dealing and checking go through the engine's batched calls.  An engine object that
    brings none of them (a CPU test double) leaves the agents on the host path, which sends the same
    messages."""
    return _gpu_dkg and all(hasattr(param.engine(), c) for c in _GPU_CALLS)


def degree(num_members: int) -> int:
    """The polynomial degree of the reference's dealing (SA_ClientAgent.py:42): int(fraction n) + 1."""
    return int(fraction * num_members) + 1


def register_dealer(agent) -> None:
    _dealers[agent.id] = agent


# ------------------------------------------------------------------ dealing
class _Recording:
    """randrange() over the agent's random state (40 bytes mod n per value, as the Flamingo clients'
    share polynomials) that remembers what it gave: shamir_share returns no coefficients."""

    def __init__(self, rs):
        self.rs, self.seen = rs, []

    def randrange(self, n):
        v = int.from_bytes(bytes(self.rs.randint(0, 256, size=40, dtype=np.uint8)), "big") % n
        self.seen.append(v)
        return v


def _draw(agent) -> list:
    """The dealer's coefficients, secret first, from its own random state: ONE draw of 40 bytes per
    coefficient, the same stream as the host path's separate draws (protocol._draw_mi says why)."""
    T = agent.poly_degree + 1
    buf = bytes(agent.random_state.randint(0, 256, size=40 * T, dtype=np.uint8))
    return [int.from_bytes(buf[40 * k: 40 * k + 40], "big") % P256_N for k in range(T)]


def _deal_host(agent) -> tuple:
    rec = _Recording(agent.random_state)
    secret = rec.randrange(P256_N)
    pts = shamir_share(secret, agent.poly_degree + 1, len(agent.users), P256_N, rng=rec)
    return ({j: pts[j - 1] for j in agent.users}, [C.mul(c) if c else None for c in rec.seen])


def deal(agent) -> tuple:
    """(shares {receiver id: (x, y)}, commitments [C_k as (x, y) or None]) of this dealer.  On the GPU
    the first dealer to ask deals for every registered dealer that has not dealt yet."""
    key = (param.root_seed, agent.id)
    if key in _dealt:
        return _dealt[key]
    if not on_gpu():
        _dealt[key] = _deal_host(agent)
        return _dealt[key]
    batch = [d for i, d in sorted(_dealers.items()) if (param.root_seed, i) not in _dealt]
    if agent.id not in [d.id for d in batch]:
        batch.append(agent)
    if any(d.poly_degree != agent.poly_degree or d.users != agent.users for d in batch):
        raise RuntimeError("the dealers of one batch share one degree and one member list")
    T, M, n = agent.poly_degree + 1, len(batch), len(agent.users)
    coeffs = [_draw(d) for d in batch]
    cw = np.frombuffer(b"".join(v.to_bytes(32, "big") for k in range(T) for co in coeffs for v in [co[k]]),
                       np.uint8).reshape(T, M, 32)
    eng = param.engine()
    shares = eng.shamir_deal_wire(cw, np.asarray(agent.users, np.uint32))          # (n, M, 32), point-major
    gw = np.tile(np.frombuffer(C.point_bytes(C.G), np.uint8), (T * M, 1))
    com, fl = eng.ec_mul_wire(gw, cw.reshape(T * M, 32))
    pts = C.points_from_wire(np.asarray(com), fl)                                   # infinity (flag bit 2) -> None
    for i, d in enumerate(batch):
        ys = [int.from_bytes(bytes(shares[c, i]), "big") for c in range(n)]
        _dealt[(param.root_seed, d.id)] = ({j: (j, ys[c]) for c, j in enumerate(agent.users)},
                                           [pts[k * M + i] for k in range(T)])
    return _dealt[key]


# ------------------------------------------------------------------ checking
def check_shares(rows, x_bits: int | None = None) -> list:
    """One verdict per (commitments [C_k], x, share) row; x_bits: the bits of x the kernel walks (the
    members pass the bit length of n), None: the bit length of the largest x.  On the GPU the rows are ONE
    flm_feldman_verify launch over the distinct commitment lists: the grid form (no dealer array) where
    every row has its own list, as a member's check of SHARE_AND_COMMIT does; else the row form."""
    rows = list(rows)
    if not rows:
        return []
    if not on_gpu():
        return [C.feldman_verify(s, x, com) for com, x, s in rows]
    lists, index = [], {}
    dealer = []
    for com, _, _ in rows:
        k = id(com)
        if k not in index:
            index[k] = len(lists)
            lists.append(com)
        dealer.append(index[k])
    T = len(lists[0])
    if any(len(com) != T for com in lists):
        raise RuntimeError("the commitment lists of one check have one length")
    cw = np.stack([C.points_to_wire([com[k] for com in lists]) for k in range(T)])   # (T, M, 64)
    grid = dealer == list(range(len(rows)))
    xs = [int(x) for _, x, _ in rows]
    sw = np.full((len(rows), 32), 0xFF, np.uint8)        # a share with no wire form: 2^256 - 1, refused
    for i, (_, _, s) in enumerate(rows):
        if isinstance(s, int) and 0 <= s < (1 << 256):
            sw[i] = np.frombuffer(s.to_bytes(32, "big"), np.uint8)
    ok, _, _ = param.engine().feldman_verify_wire(cw, None if grid else dealer, xs, sw,
                                                  x_bits=x_bits or max(1, max(xs).bit_length()))
    return [bool(v) for v in ok]


def group_key(constant_terms):
    """sum of the C_{i,0} over QUAL (the reference never computes it): one flm_ec_combine with every
    coefficient 1, no base point and no negation; infinity terms (a zero secret) add nothing."""
    pts = [p for p in constant_terms if p is not None]
    if not pts:
        return None
    if not on_gpu():
        acc = None
        for p in pts:
            acc = C.add(acc, p)
        return acc
    sw = C.points_to_wire(pts).reshape(len(pts), 1, 64)
    out, _, fl = param.engine().ec_combine_wire(None, sw, C.scalars_to_wire([1] * len(pts)), negate=False)
    return C.points_from_wire(np.asarray(out), fl)[0]
