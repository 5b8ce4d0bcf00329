"""Deterministic inputs that steer the GPU inversion (flamingo_amd/csrc/flm_fe256.h inv_bingcd:
Pornin's binary GCD, 18 outer steps of 30 inner steps) and the ECDSA kernel's joint regular ladder
(flm_p256.hip ecdsa_verify_kernel) into branches no random input reaches.  No test functions: the
premises are checked without a GPU by tests/test_inv_cases_cpu.py, the kernels against the rows by
tests/test_inv_edges_gpu.py.  Which branch an input takes is read from the trace of
tools/bingcd_model.py, the one Python statement of the schedule; expected values come from
oracle/ec_oracle.py and Python integers.

Lists of inverter inputs (Inv tuples: name, x, and from the model's trace the outer steps to a == 0,
the outer steps to b == 1 and the outer steps of the two negations), for mod = p and mod = n:

* slow_inputs(mod): inputs c << k and mod - (c << k) whose run needs 15, 16, 17 and all 18 outer
  steps to a == 0 (random inputs need 12 to 14).  Every 18-step input of the scan c odd, k in
  243..255 is there, 2^255 among them: 10 mod p (4593<<243, 8149<<243, 2299<<244, 2753<<244,
  1111<<245, 1301<<245, 923<<246, 71<<249, 13<<252, 2^255) and 13 mod n (7161<<243, 7581<<243,
  3929<<244, 1489<<245, 627<<246, 341<<247, 361<<247, 431<<247, 133<<248, 57<<250, 21<<251, 31<<251,
  2^255), and SLOW_PER_STEP = 12 each at 15, 16 and 17 steps (k from 255 down: about 30 bits of k to
  the step).  No input of any family here needs 19.
  What the kernel returns is v, which is final once b == 1 (`settled`): from then on only a and u
  change.  That is at least one inner step before a == 0, and every input found, the 18-step ones
  included, settles by outer step 17 (2^255, and the other pure powers of two, by step 9): 16 inputs
  mod p and 19 mod n settle at 17, none at 18.  If the algorithm's bound of 2 * 256 - 1 = 511 inner
  steps to a == 0 holds for this variant, b == 1 by inner step 510 = 17 * 30 always, and the 18th
  outer step only takes a to 0.  So these inputs tell a 16-step kernel from the real one, not a
  17-step kernel: no known input does.
* tied_inputs(mod): the inputs of the family mod - c 2^j + off (j in 31..221, c in 1, 3, 5, off in
  TIED_OFFSETS) at which the approximations order a and b wrongly (their 34-bit top windows tie
  while the dropped middle bits differ), so a or b comes out negative and the nga / ngb branch
  negates it with its matrix row.  The family (5157 inputs per modulus) takes nga 497 times and ngb
  47 times mod p, nga 480 times and ngb 1920 times mod n; the list keeps TIED_PER_SITE = 8 of each
  (branch, outer step, window index q): 24 nga and 39 ngb inputs mod p, 8 and 8 mod n.
    - mod n every negation is at outer step 1 in the aligned window q = 6: none at a later step
      was found, in the family or in 60,000 random inputs, and mod n the later sites are not
      reached by anything here.
    - mod p nga is also taken at the (outer step, q) pairs (3, 4), (4, 3), (5, 2), (6, 1), (6, 2),
      (7, 0), (7, 1) and ngb at (4, 3), (5, 2), (6, 1), (6, 2), (7, 0), (7, 1), (9, 0), all in
      unaligned windows; step 1 (q = 6, aligned) is nga only.  Mod p the branches are not as rare as
      a 2^-34 tie: about 1 random input in 20,000 takes one (the den of hash to curve's message
      "32004" takes nga at step 5), so the 65,536-point table of tests/test_h2c_gpu.py crosses them
      by chance; these lists cross every known site on purpose, in a few lanes.
  A wrong sign of the inverse cannot show in an ECDSA verdict: -w turns R into -R, and x(-R) = x(R).
  Leaving out nga's sign flip at outer step 1 does exactly that, so the mod-n nga rows pin the
  value of w up to sign only; the same template's sign is pinned mod p, where the den's inverse
  decides the point.  (Leaving out ngb's does change the verdicts mod n.)
* quotient_inputs(mod): seeded random inputs (10 mod p, 13 mod n) that between them put a
  bg_lin_modp quotient in each of the four ranges [-m, 0), [0, m), [m, 2^256), [2^256, 2m] (the
  kernel's three fix-ups and the plain path; the rarest occurs about 90 times in 2000 random runs)
  twice, and one input for every window index q = 0..6 at sh & 31 == 0 (q = 5 aligned is the
  rarest, 3 in 2000).

mod n these reach the kernel as the s of a signature: ecdsa_row_for_s(s, label) is a valid
digest-level signature with that s (key and nonce from the label, e = s k - r d), expected verdict
from the plain-Python FIPS 186-4 `verify` below, with a twin whose digest has one bit flipped.

mod p they reach it as h2c_map's den: uniform_for_den(A) is the 48-byte half whose u makes
den = 100 u^4 - 10 u^2 in Montgomery form the integer A (about 3 targets in 8 have a solution);
den_rows() pairs each solved half with an ordinary one in both lane orders.  The solved pool
(den_pool(), 40 targets) holds 4 at 18 steps (923<<246, 2299<<244, 4593<<243, 8149<<243; 2^255 and
13<<252 have no solution), 5 at 17, 5 at 16 and 3 at 15, 6 of them settling at step 17; and up to
DEN_PER_SITE = 3 per negation site, 10 that take nga and 13 that take ngb, at every (outer step, q)
pair listed above but nga (7, 0), nga (7, 1) and ngb (7, 1), whose four family members have no
solution.

Not reached, because nothing outside the kernels sets it: the Z that ec_finish_kernel and
feldman_verify_kernel invert and the R.Z of h2c_tail (each a product of the whole chain before it,
in effect random).  They call the same fe_inv_bingcd as the den path, which is the mod-p instance
that can be steered.

The ladder: regular_digits / ladder_events restate regular_recode / regular_next and the kernel's
loop on scalars mod n (Q = d G), and ladder_row(kind, which, window, label) solves the key d for
which the accumulator meets the addend ("double": acc == addend, "infinity": acc == -addend) at the
G addition (jac_add_affine from kGOdd) or the Q addition (jac_add from the lane's table) of that
window.  An "infinity" event is followed by an addition to an accumulator at infinity
("from-infinity"), at the Q addition of the same window or the G addition of the next.
ladder_rows() covers both additions, both kinds, windows 0, 1, 31, 62 and 63, but for ("infinity",
"Q", 63): that is the last addition, its sum is the final result, and the row would be the
fixture's sum-at-infinity case (flag bit 2), not a valid signature.
"""
from __future__ import annotations

import functools
import hashlib
import os
import random
import sys
from collections import namedtuple

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _d in ("oracle", "tools", "tests"):
    if os.path.join(_ROOT, _d) not in sys.path:
        sys.path.insert(0, os.path.join(_ROOT, _d))

import bingcd_model as M  # noqa: E402
import ec_oracle as E  # noqa: E402
import h2c_cases as H  # noqa: E402

P, N = E.P, E.N
R = 2**256
R_INV = pow(R, -1, P)

Inv = namedtuple("Inv", "name x steps settled nga ngb")     # steps: to a == 0, settled: to b == 1 (the result
                                                            # final); nga, ngb: tuples of outer steps (from 1)


def traced(x: int, mod: int) -> dict:
    """The model's trace of x; the model's own assertions (a == 0, b == 1 after 18 steps) hold and
    its result is the inverse."""
    tr = {}
    assert M.inv(x, trace=tr, mod=mod) == pow(x, -1, mod), x
    return tr


def _inv_case(name: str, x: int, mod: int) -> Inv:
    tr = traced(x, mod)
    return Inv(name, x, tr["done"], tr["settled"], tuple(tr["nga"]), tuple(tr["ngb"]))


def _mod_name(mod: int) -> str:
    return {P: "p", N: "n"}[mod]


# ------------------------------------------------------------------ slow inputs
SLOW_PER_STEP = 12


@functools.lru_cache(maxsize=None)
def slow_inputs(mod: int) -> tuple:
    m = _mod_name(mod)
    by = {15: [], 16: [], 17: [], 18: []}
    # every 18-step input among c << k, c odd, k in 243..255 (2^255 is c = 1, k = 255)
    for k in range(243, 256):
        for c in range(1, 1 << (256 - k), 2):
            if c << k < mod and traced(c << k, mod)["done"] == 18:
                by[18].append(_inv_case(f"{c}<<{k}", c << k, mod))
    # 15, 16, 17 (and further 18s) from small odd c over k in 160..255, plain and subtracted from mod:
    # each 30 bits of k cost one outer step (17 from k near 225 up, 16 near 195..224, 15 near 165..194)
    for k in range(255, 159, -1):
        for c in (1, 3, 5, 7, 11, 13, 21, 31):
            for name, x in ((f"{c}<<{k}", c << k), (f"{m}-({c}<<{k})", mod - (c << k))):
                if not 0 < x < mod:
                    continue
                case = _inv_case(name, x, mod)
                if case.steps in by and case.x not in {i.x for i in by[case.steps]} and \
                        (case.steps == 18 or len(by[case.steps]) < SLOW_PER_STEP):
                    by[case.steps].append(case)
    return tuple(by[15] + by[16] + by[17] + by[18])


# ------------------------------------------------------------------ tied top windows: the negations
TIED_OFFSETS = (0, 2, -2, 4, -4, 6, -6, 1024, -1024)
TIED_PER_SITE = 8


@functools.lru_cache(maxsize=None)
def tied_family(mod: int) -> tuple:
    """Every member of mod - c 2^j + off that takes nga or ngb, as (Inv, sites): sites is the set of
    (branch, outer step, q) at which it negates."""
    m, out = _mod_name(mod), []
    for j in range(31, 222):
        for c in (1, 3, 5):
            for off in TIED_OFFSETS:
                x = mod - c * 2**j + off
                tr = traced(x, mod)
                if tr["nga"] or tr["ngb"]:
                    sites = {("nga", s, tr["windows"][s - 1][0]) for s in tr["nga"]} | \
                            {("ngb", s, tr["windows"][s - 1][0]) for s in tr["ngb"]}
                    name = f"{m}-{c}*2^{j}{off:+d}"
                    out.append((_inv_case(name, x, mod), frozenset(sites)))
    return tuple(out)


def _per_site(family, per_site: int) -> tuple:
    """The first per_site members of `family` ((Inv, sites) pairs) at every site."""
    count, out = {}, []
    for case, sites in family:
        if any(count.get(s, 0) < per_site for s in sites):
            out.append(case)
            for s in sites:
                count[s] = count.get(s, 0) + 1
    return tuple(out)


@functools.lru_cache(maxsize=None)
def tied_inputs(mod: int) -> tuple:
    return _per_site(tied_family(mod), TIED_PER_SITE)


def tied_sites(mod: int) -> dict:
    """{(branch, outer step, q): how many members of the family negate there}"""
    out = {}
    for _, sites in tied_family(mod):
        for s in sites:
            out[s] = out.get(s, 0) + 1
    return out


# ------------------------------------------------------------------ quotient ranges, aligned windows
@functools.lru_cache(maxsize=None)
def quotient_inputs(mod: int) -> tuple:
    """Seeded random inputs, kept while they add a bg_lin_modp range (two of each) or an aligned
    window index not yet seen."""
    rng = random.Random(4100 + (mod == N))
    ranges, aligned, out = {r: 0 for r in M.QUOT_RANGES}, set(), []
    for i in range(20000):
        if min(ranges.values()) >= 2 and aligned == set(range(7)):
            break
        x = rng.randrange(1, mod)
        tr = traced(x, mod)
        new_r = {r for pair in tr["quot"] for r in pair if ranges[r] < 2}
        new_q = {q for q, al in tr["windows"] if al} - aligned
        if new_r or new_q:
            for r in new_r:
                ranges[r] += 1
            aligned |= new_q
            what = ",".join(sorted(new_r) + [f"q{q}" for q in sorted(new_q)])
            out.append(_inv_case(f"random {i} ({what})", x, mod))
    assert min(ranges.values()) >= 2 and aligned == set(range(7))
    return tuple(out)


# ------------------------------------------------------------------ ECDSA rows
def h_int(label: str) -> int:
    return int.from_bytes(hashlib.sha256(label.encode()).digest(), "big")


def b32(v: int) -> bytes:
    return int(v).to_bytes(32, "big")


def verify(q: bytes, e: bytes, r: int, s: int):
    """(verdict, flags) of one row by FIPS 186-4 section 6.4.2 on the oracle's affine arithmetic.
    flags bit 0: r or s outside [1, n-1], bit 1: q not a valid point, bit 2: u1 G + u2 Q at infinity."""
    flags = 0
    if not (1 <= r < N and 1 <= s < N):
        flags |= 1
    x, y = int.from_bytes(q[:32], "big"), int.from_bytes(q[32:], "big")
    if x >= P or y >= P or not E.on_curve((x, y)) or q == bytes(64):
        flags |= 2
    if flags:
        return False, flags
    w = pow(s, -1, N)
    u1, u2 = int.from_bytes(e, "big") % N * w % N, r * w % N
    pt = E.add(E.mul(u1), E.mul(u2, (x, y)))
    if pt is None:
        return False, 4
    return pt[0] % N == r, 0


def _case(name: str, q: bytes, e: bytes, r: int, s: int) -> dict:
    ok, flags = verify(q, e, r, s)
    return {"name": name, "q": q.hex(), "e": e.hex(), "r": b32(r).hex(), "s": b32(s).hex(), "ok": ok, "flags": flags}


def _with_twin(name: str, q: bytes, e: bytes, r: int, s: int) -> tuple:
    """the row and its twin with one bit of the digest flipped (2^b is not 0 mod n: another e mod n)"""
    bit = h_int(f"bit:{name}") % 256
    flipped = bytearray(e)
    flipped[bit >> 3] ^= 1 << (bit & 7)
    row, twin = _case(name, q, e, r, s), _case(name + "/e-bit", q, bytes(flipped), r, s)
    assert (row["ok"], row["flags"], twin["ok"], twin["flags"]) == (True, 0, False, 0), name
    return row, twin


@functools.lru_cache(maxsize=None)
def ecdsa_row_for_s(s: int, label: str) -> tuple:
    """(row, twin): a valid signature (r, s) with the chosen s under a key and a nonce derived from
    the label: r = x(k G) mod n and the digest e = s k - r d mod n."""
    assert 0 < s < N
    ctr = 0
    while True:
        d = h_int(f"key:{label}:{ctr}") % (N - 1) + 1
        k = h_int(f"nonce:{label}:{ctr}") % (N - 1) + 1
        r = E.mul(k)[0] % N
        if r:
            break
        ctr += 1
    return _with_twin(label, E.wire(E.mul(d)), b32((s * k - r * d) % N), r, s)


@functools.lru_cache(maxsize=None)
def inverter_rows() -> tuple:
    """(row, twin) for every mod-n inverter input: the slow, the tied and the quotient inputs."""
    out = []
    for fam, cases in (("slow", slow_inputs(N)), ("tied", tied_inputs(N)), ("quot", quotient_inputs(N))):
        out += [ecdsa_row_for_s(c.x, f"{fam} s={c.name}") for c in cases]
    return tuple(out)


@functools.lru_cache(maxsize=None)
def ordinary_rows() -> tuple:
    """16 ordinary signatures, valid and digest-tampered alternating: the neighbours in mixed batches"""
    out = []
    for i in range(8):
        s = h_int(f"ordinary-s:{i}") % (N - 1) + 1
        out += ecdsa_row_for_s(s, f"ordinary {i}")
    return tuple(out)


# ------------------------------------------------------------------ hash to curve's den
def uniform_for_den(A: int):
    """The 48-byte half whose u < n gives den R mod p == A (what fe_inv_bingcd receives), or None:
    with D = A / R, t = u^2 solves 100 t^2 - 10 t = D, i.e. t = (10 +- sqrt(100 + 400 D)) / 200."""
    assert 0 < A < P
    D = A * R_INV % P
    root = pow(100 + 400 * D, (P + 1) // 4, P)
    if root * root % P != (100 + 400 * D) % P:
        return None
    for sq in (root, P - root):
        t = (10 + sq) * pow(200, -1, P) % P
        u = pow(t, (P + 1) // 4, P)
        if u * u % P != t:
            continue
        if u >= N:
            u = P - u
        if 0 < u < N:
            return H.half(u)
    return None


DEN_PER_STEP = 8
DEN_PER_SITE = 3
Den = namedtuple("Den", "case half sites")          # case: Inv (x = A), half: 48 bytes, sites: as tied_family


@functools.lru_cache(maxsize=None)
def den_pool() -> tuple:
    """The mod-p targets that have a solution: the slow inputs (every 18-step one, DEN_PER_STEP at
    each lower count) and up to DEN_PER_SITE of the tied family per negation site."""
    out, steps = [], {}
    for c in slow_inputs(P):
        h = uniform_for_den(c.x)
        if h is not None and (c.steps == 18 or steps.get(c.steps, 0) < DEN_PER_STEP):
            steps[c.steps] = steps.get(c.steps, 0) + 1
            out.append(Den(c, h, frozenset()))
    solved = [(c, sites, uniform_for_den(c.x)) for c, sites in tied_family(P)]
    solved = [(c, sites, h) for c, sites, h in solved if h is not None]
    keep = {c.x for c in _per_site([(c, sites) for c, sites, _ in solved], DEN_PER_SITE)}
    out += [Den(c, h, sites) for c, sites, h in solved if c.x in keep]
    return tuple(out)


DenRow = namedtuple("DenRow", "name ub A lane")


@functools.lru_cache(maxsize=None)
def den_rows() -> tuple:
    """Every solved half beside an ordinary seeded half, in both lane orders."""
    out = []
    for k, dn in enumerate(den_pool()):
        o = H.half(H.ordinary(9000 + k))
        out.append(DenRow(f"den {dn.case.name} | ord", dn.half + o, dn.case.x, 0))
        out.append(DenRow(f"den ord | {dn.case.name}", o + dn.half, dn.case.x, 1))
    return tuple(out)


def den_ordinary(i: int) -> DenRow:
    return DenRow(f"ord {i}", H.half(H.ordinary(9500 + i)) + H.half(H.ordinary(9700 + i)), None, None)


def den_of(half: bytes) -> int:
    """den R mod p of the u a half reduces to, by the oracle's formula den = 100 u^4 - 10 u^2"""
    u = int.from_bytes(half, "big") % N
    return (100 * pow(u, 4, P) - 10 * pow(u, 2, P)) * R % P


# ------------------------------------------------------------------ the ladder
def regular_digits(k: int):
    """regular_recode / regular_next of a scalar k < n: (sign, 64 odd digits in [-15, 15] from the
    top), k = sign (2^256 + sum d_i 16^(63 - i)) mod n.  An even k (0 included) is recoded as
    n - k with the sign flipped."""
    assert 0 <= k < N
    neg = k % 2 == 0
    h = (N - k if neg else k) >> 1
    digs = []
    for _ in range(64):
        digs.append(2 * (h >> 252) - 15)
        h = (h << 4) & (R - 1)
    return (-1 if neg else 1), digs


def ladder_events(u1: int, u2: int, d: int) -> list:
    """The kernel's joint ladder for u1 G + u2 Q, Q = d G, on scalars mod n: acc = +-Q, then + (+-G)
    (the top digits; reported as window -1), then per window four doublings, + (digit of u1) G,
    + (digit of u2) Q.  Returns [(window, "G" or "Q", kind)] for every addition whose accumulator
    equals the addend ("double"), its negative ("infinity") or is at infinity ("from-infinity")."""
    (s1, d1), (s2, d2) = regular_digits(u1), regular_digits(u2)
    events = []

    def add(acc, addend, w, which):
        if acc == 0:
            events.append((w, which, "from-infinity"))
        elif acc == addend % N:
            events.append((w, which, "double"))
        elif acc == -addend % N:
            events.append((w, which, "infinity"))
        return (acc + addend) % N

    acc = add(s2 * d % N, s1, -1, "G")
    for w in range(64):
        acc = 16 * acc % N
        acc = add(acc, s1 * d1[w], w, "G")
        acc = add(acc, s2 * d2[w] * d, w, "Q")
    assert acc == (u1 + u2 * d) % N
    return events


LADDER_WINDOWS = (0, 1, 31, 62, 63)
LADDER_KINDS = tuple((kind, which, w) for which in "GQ" for kind in ("double", "infinity") for w in LADDER_WINDOWS
                     if (kind, which, w) != ("infinity", "Q", 63))          # the last addition: the sum itself


@functools.lru_cache(maxsize=None)
def ladder_row(kind: str, which: str, window: int, label: str) -> tuple:
    """(row, twin, d, events): a valid signature whose verification meets `kind` at the `which`
    addition of `window`; events is ladder_events' whole list for it."""
    ctr = 0
    while True:
        u1 = h_int(f"ladder-u1:{label}:{ctr}") % (N - 1) + 1
        u2 = h_int(f"ladder-u2:{label}:{ctr}") % (N - 1) + 1
        ctr += 1
        (s1, d1), (s2, d2) = regular_digits(u1), regular_digits(u2)
        a, b = s1, s2                    # acc = a + b d before the window's doublings
        for w in range(window):
            a, b = 16 * a + s1 * d1[w], 16 * b + s2 * d2[w]
        g, q = s1 * d1[window], s2 * d2[window]
        sign = 1 if kind == "double" else -1
        if which == "G":                 # 16 (a + b d) = +-g
            num, den = sign * g * pow(16, -1, N) - a, b
        else:                            # 16 (a + b d) + g = +-q d
            num, den = -(16 * a + g), 16 * b - sign * q
        if den % N == 0:
            continue
        d = num * pow(den, -1, N) % N
        pt = E.mul((u1 + u2 * d) % N)
        if d == 0 or pt is None or pt[0] % N == 0:
            continue
        r = pt[0] % N
        s = r * pow(u2, -1, N) % N
        events = ladder_events(u1, u2, d)
        assert (window, which, kind) in events, (label, events)
        return _with_twin(label, E.wire(E.mul(d)), b32(u1 * s % N), r, s) + (d, tuple(events))


@functools.lru_cache(maxsize=None)
def ladder_rows() -> tuple:
    return tuple(ladder_row(kind, which, w, f"ladder {kind} {which} {w}") for kind, which, w in LADDER_KINDS)
