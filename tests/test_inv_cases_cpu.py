"""The premises of tests/inv_cases.py, without a GPU: every listed inverter input inverts in the model
(tools/bingcd_model.py) and takes the branch it is listed for, the counts the lists promise hold for
both moduli, every solved hash-to-curve half reproduces its target den, every ECDSA row has its
stated verdict from the plain-Python verify and from OpenSSL, ladder_events agrees with a walk of
the same ladder on affine points, and a structured search finds no input that needs a 19th step."""
from __future__ import annotations

import functools

import pytest

import ec_oracle as E
import inv_cases as C

M = C.M                                  # tools/bingcd_model.py, on the path inv_cases set up

P, N = E.P, E.N
MODULI = pytest.mark.parametrize("mod", [P, N], ids=["p", "n"])


# ------------------------------------------------------------------ the inverter lists
@MODULI
def test_every_listed_input_inverts_in_the_model(mod):
    cases = C.slow_inputs(mod) + C.tied_inputs(mod) + C.quotient_inputs(mod)
    assert len({c.x for c in cases}) == len(cases)
    for c in cases:
        assert 0 < c.x < mod
        tr = {}
        assert M.inv(c.x, trace=tr, mod=mod) == pow(c.x, -1, mod), c.name
        assert (tr["done"], tr["settled"], tuple(tr["nga"]), tuple(tr["ngb"])) == (c.steps, c.settled, c.nga, c.ngb), c.name
        assert len(tr["windows"]) == len(tr["quot"]) == 18 and all(0 <= q <= 6 for q, _ in tr["windows"])


@MODULI
def test_slow_inputs_cover_15_to_18_steps(mod):
    cases = C.slow_inputs(mod)
    count = {s: sum(c.steps == s for c in cases) for s in (15, 16, 17, 18)}
    assert min(count[15], count[16], count[17]) >= 8 and count[18] >= 3, count
    assert all(c.steps in count and c.settled <= min(c.steps, 17) for c in cases)
    # what a shorter schedule would get wrong is v, final at `settled`: these tell 16 outer steps from 18
    assert sum(c.settled == 17 for c in cases) >= 8
    xs = {c.x for c in cases}
    assert 1 << 255 in xs
    # every 18-step input of the scan the list's docstring names, re-derived here
    scan = {c << k for k in range(243, 256) for c in range(1, 1 << (256 - k), 2)
            if c << k < mod and C.traced(c << k, mod)["done"] == 18}
    assert scan <= xs and len(scan) == {P: 10, N: 13}[mod]
    named = {P: [(923, 246), (13, 252), (2299, 244), (4593, 243), (8149, 243)], N: [(21, 251), (31, 251)]}[mod]
    assert {c << k for c, k in named} <= scan


@MODULI
def test_tied_inputs_take_the_negation_branches(mod):
    cases = C.tied_inputs(mod)
    nga, ngb = [c for c in cases if c.nga], [c for c in cases if c.ngb]
    assert len(nga) >= 8 and len(ngb) >= 2 and all(c.nga or c.ngb for c in cases)
    # the inputs the list's docstring is built on
    assert C.traced(mod - 2**100, mod)["nga"] == [1]
    assert C.traced(N - 2**31 + 2, N)["ngb"] == [1] and C.traced(P - 2**178 + 1024, P)["ngb"]
    sites = C.tied_sites(mod)
    family = C.tied_family(mod)
    assert (sum(1 for c, _ in family if c.nga), sum(1 for c, _ in family if c.ngb)) == {P: (497, 47), N: (480, 1920)}[mod]
    # the list has a member at every site the family reaches
    listed = {(b, s, C.traced(c.x, mod)["windows"][s - 1][0]) for c in cases for b, ss in (("nga", c.nga), ("ngb", c.ngb))
              for s in ss}
    assert listed == set(sites)
    if mod == N:
        assert set(sites) == {("nga", 1, 6), ("ngb", 1, 6)}          # mod n: outer step 1 only
    else:
        assert {(b, s, q) for b, s, q in sites if s > 1} == \
            {("nga", 3, 4), ("nga", 4, 3), ("nga", 5, 2), ("nga", 6, 1), ("nga", 6, 2), ("nga", 7, 0), ("nga", 7, 1),
             ("ngb", 4, 3), ("ngb", 5, 2), ("ngb", 6, 1), ("ngb", 6, 2), ("ngb", 7, 0), ("ngb", 7, 1), ("ngb", 9, 0)}


@MODULI
def test_quotient_inputs_reach_every_range_and_aligned_window(mod):
    ranges, aligned, short, pow30 = set(), set(), 0, 0
    for c in C.quotient_inputs(mod):
        tr = C.traced(c.x, mod)
        ranges |= {r for pair in tr["quot"] for r in pair}
        aligned |= {q for q, al in tr["windows"] if al}
        short += len(tr["short"])
        pow30 += len(tr["pow30"])
        assert tr["short"] == list(range(tr["short"][0], 19))         # once short, short to the end
    assert ranges == set(M.QUOT_RANGES) and aligned == set(range(7)) and short and pow30


def test_trace_keeps_its_old_field_and_return_value():
    tr = {}
    x = C.h_int("an ordinary input") % P
    assert M.inv(x, trace=tr) == pow(x, -1, P) == M.inv(x)
    assert set(tr) == {"done", "settled", "nga", "ngb", "windows", "short", "pow30", "quot"} and 1 <= tr["done"] <= 18
    assert tr["windows"][0] == (6, True) and tr["quot"][0] == ("plain", "plain")


# ------------------------------------------------------------------ hash to curve's den
def test_uniform_for_den_reproduces_its_targets():
    pool = C.den_pool()
    for dn in pool:
        assert len(dn.half) == 48 and 0 < int.from_bytes(dn.half, "big") < N
        assert C.den_of(dn.half) == dn.case.x, dn.case.name
        tr = C.traced(dn.case.x, P)
        assert (tr["done"], tuple(tr["nga"]), tuple(tr["ngb"])) == (dn.case.steps, dn.case.nga, dn.case.ngb)
    slow = [dn.case.steps for dn in pool if not dn.sites]
    assert slow.count(18) >= 2 and slow.count(16) + slow.count(17) >= 8
    assert sum(1 for dn in pool if dn.case.nga) >= 4 and sum(1 for dn in pool if dn.case.ngb) >= 1
    assert {dn.case.name for dn in pool if dn.case.steps == 18 and not dn.sites} == \
        {"923<<246", "2299<<244", "4593<<243", "8149<<243"}
    # what has no solution says so
    assert C.uniform_for_den(1 << 255) is None and C.uniform_for_den(13 << 252) is None


def test_den_rows_put_each_half_in_both_lanes():
    rows = C.den_rows()
    assert len(rows) == 2 * len(C.den_pool())
    for r in rows:
        assert len(r.ub) == 96 and C.den_of(r.ub[48 * r.lane: 48 * r.lane + 48]) == r.A
        assert C.den_of(r.ub[48 * (1 - r.lane): 48 * (2 - r.lane)]) != r.A
        wire, flag = C.H.expect(r.ub)
        assert flag == 0 and any(wire)


# ------------------------------------------------------------------ the ECDSA rows
@functools.lru_cache(maxsize=None)
def all_rows():
    return tuple(r for pair in C.inverter_rows() for r in pair) + C.ordinary_rows() + \
        tuple(r for row in C.ladder_rows() for r in row[:2])


def test_inverter_rows_carry_the_listed_s():
    want = [c.x for c in C.slow_inputs(N) + C.tied_inputs(N) + C.quotient_inputs(N)]
    assert [int(row["s"], 16) for row, _ in C.inverter_rows()] == want
    assert [int(twin["s"], 16) for _, twin in C.inverter_rows()] == want


def test_rows_have_their_verdicts_in_plain_python_and_openssl():
    from flamingo_amd import crypto
    rows = all_rows()
    assert len({r["name"] for r in rows}) == len(rows)
    for r in rows:
        q, e, sig = bytes.fromhex(r["q"]), bytes.fromhex(r["e"]), bytes.fromhex(r["r"] + r["s"])
        assert C.verify(q, e, int(r["r"], 16), int(r["s"], 16)) == (r["ok"], 0) and r["flags"] == 0, r["name"]
        assert r["ok"] == (not r["name"].endswith("/e-bit"))
        pub = (int.from_bytes(q[:32], "big"), int.from_bytes(q[32:], "big"))
        assert crypto.ecdsa_verify_digest(pub, e, sig) == r["ok"], r["name"]


# ------------------------------------------------------------------ the ladder
def test_regular_digits_reproduce_the_scalar():
    for k in (0, 1, 2, 3, 15, 16, 17, N - 1, N - 2, N - 3, (N - 1) // 2, 1 << 255, (1 << 255) + 1):
        sign, digs = C.regular_digits(k)
        assert len(digs) == 64 and all(d % 2 and -15 <= d <= 15 for d in digs)
        acc = 1
        for d in digs:
            acc = 16 * acc + d
        assert (sign * acc - k) % N == 0 and acc < (1 << 257), k


def walk(u1: int, u2: int, Q) -> tuple:
    """The same ladder on affine points with the oracle's add: (events, result)"""
    (s1, d1), (s2, d2) = C.regular_digits(u1), C.regular_digits(u2)
    signed = lambda pt, v: pt if v > 0 else E.neg(pt)  # noqa: E731
    tab_g = [E.mul(2 * t + 1) for t in range(8)]
    tab_q = [E.mul(2 * t + 1, Q) for t in range(8)]
    events = []

    def add(acc, addend, w, which):
        if acc is None:
            events.append((w, which, "from-infinity"))
        elif acc == addend:
            events.append((w, which, "double"))
        elif acc == E.neg(addend):
            events.append((w, which, "infinity"))
        return E.add(acc, addend)

    acc = add(signed(Q, s2), signed(E.G, s1), -1, "G")
    for w in range(64):
        for _ in range(4):
            acc = E.add(acc, acc)
        acc = add(acc, signed(tab_g[abs(d1[w]) >> 1], s1 * d1[w]), w, "G")
        acc = add(acc, signed(tab_q[abs(d2[w]) >> 1], s2 * d2[w]), w, "Q")
    return events, acc


def test_ladder_rows_meet_their_events_on_affine_points():
    rows = C.ladder_rows()
    assert len(rows) == 19 and len(C.LADDER_KINDS) == 19
    for (kind, which, w), (row, twin, d, events) in zip(C.LADDER_KINDS, rows):
        q = bytes.fromhex(row["q"])
        Q = (int.from_bytes(q[:32], "big"), int.from_bytes(q[32:], "big"))
        assert Q == E.mul(d)
        r, wi = int(row["r"], 16), pow(int(row["s"], 16), -1, N)
        u1, u2 = int(row["e"], 16) % N * wi % N, r * wi % N
        got, result = walk(u1, u2, Q)
        assert tuple(got) == events == tuple(C.ladder_events(u1, u2, d)), row["name"]
        assert result is not None and result[0] % N == r
        # exactly the requested event, and after an "infinity" the addition that starts again from infinity
        after = {"G": (w, "Q"), "Q": (w + 1, "G")}[which] + ("from-infinity",)
        assert list(events) == [(w, which, kind)] + ([after] if kind == "infinity" else []), row["name"]
    # an ordinary signature meets none
    row = C.ordinary_rows()[0]
    wi = pow(int(row["s"], 16), -1, N)
    q = bytes.fromhex(row["q"])
    assert walk(int(row["e"], 16) % N * wi % N, int(row["r"], 16) * wi % N,
                (int.from_bytes(q[:32], "big"), int.from_bytes(q[32:], "big")))[0] == []


def test_ladder_events_of_the_fixtures_edge_keys():
    """what the ECDSA fixture already reaches: keys +-1 meet G at the top digits; u1 G == u2 Q meets
    nothing, since the joint ladder never holds the two products apart"""
    assert C.ladder_events(5, 5, 1) == [(-1, "G", "double")]
    assert C.ladder_events(5, 5, N - 1)[0] == (-1, "G", "infinity")
    t = C.h_int("dbl:t") % (N - 1) + 1
    d = C.h_int("key:infinity") % (N - 1) + 1
    assert C.ladder_events(t, t * pow(d, -1, N) % N, d) == []                              # u1 G == u2 Q


# ------------------------------------------------------------------ the search
@MODULI
def test_structured_search_finds_no_input_that_needs_a_19th_step(mod):
    """About 24k further inputs per modulus: c << k and mod - (c << k) for 20 odd c and every k,
    mod - c 2^j + off for c in 7, 9, 11, 13 and further offsets, and the modular inverse of each.
    None trips the model's a == 0, b == 1 assertion after 18 steps, each matches pow(x, -1, mod), and
    the slowest needs all 18 to a == 0 but has b == 1, and with it the result, after 17.  An input
    that settles only at step 18 would be the first to tell a 17-step kernel from this one: add it
    to slow_inputs."""
    xs = set()
    for c in range(1, 40, 2):
        for k in range(256):
            xs |= {x for x in (c << k, mod - (c << k)) if 0 < x < mod}
    for c in (7, 9, 11, 13):
        for j in range(31, 222):
            xs |= {mod - c * 2**j + off for off in (0, 2, -2, 8, -8, 1 << 20)}
    xs |= {pow(x, -1, mod) for x in xs}
    assert 20000 <= len(xs) <= 30000
    worst, settled, neg = 0, 0, 0
    for x in sorted(xs):
        tr = C.traced(x, mod)
        worst, settled = max(worst, tr["done"]), max(settled, tr["settled"])
        assert tr["settled"] < tr["done"] or tr["done"] == tr["settled"] <= 17
        neg += bool(tr["nga"] or tr["ngb"])
    assert worst == 18 and settled == 17 and neg > 100
