"""CPU checks of the host-copy layout (csrc/flm_host_layout.h) through the ctx-less flm_host_layout
export (flm_internal.h, not the public header; no GPU needed).

Every array a host-pointer call moves is one span (row width in bytes, rows, may run in place).  The
layout routes each span -- in place in the pinned bounce buffer, packed there for one DMA, or
through the staging ring -- and packs the bounce buffer.  One size per span decides its route and
sizes its space, so a span can never be routed on one size and copied at another."""
import ctypes
import itertools

import numpy as np
import pytest

IN_PLACE, BOUNCE, RING = 0, 1, 2
STAGE = 32 << 20


def up(v, m):
    return (v + m - 1) // m * m


def layout(spans):
    """spans: (rows, width, may_in_place) -> ([(route, pitch, offset)], total)"""
    from flamingo_amd import _lib
    fn = _lib.load().flm_host_layout
    u64p = ctypes.POINTER(ctypes.c_uint64)
    intp = ctypes.POINTER(ctypes.c_int)
    fn.restype = ctypes.c_int
    fn.argtypes = [ctypes.c_int, u64p, u64p, intp, intp, u64p, u64p, u64p]
    n = len(spans)
    width = np.array([s[1] for s in spans], np.uint64)
    rows = np.array([s[0] for s in spans], np.uint64)
    may = np.array([1 if s[2] else 0 for s in spans], np.intc)
    route = np.zeros(n, np.intc)
    pitch, offset = np.zeros(n, np.uint64), np.zeros(n, np.uint64)
    total = ctypes.c_uint64()
    assert fn(n, width.ctypes.data_as(u64p), rows.ctypes.data_as(u64p), may.ctypes.data_as(intp),
              route.ctypes.data_as(intp), pitch.ctypes.data_as(u64p), offset.ctypes.data_as(u64p),
              ctypes.byref(total)) == 0
    return [(int(route[i]), int(pitch[i]), int(offset[i])) for i in range(n)], int(total.value)


def room(span, placed):
    """Bounce bytes the span occupies, from its route and pitch alone."""
    rows, width, _ = span
    route, pitch, _ = placed
    if route == RING:
        return 0
    return up(rows * pitch, 256) if route == IN_PLACE else up(rows * width, 256)


def check_properties(spans):
    placed, total = layout(spans)
    end = 0
    for span, p in zip(spans, placed):
        rows, width, may = span
        route, pitch, offset = p
        assert route in (IN_PLACE, BOUNCE, RING)
        assert offset % 256 == 0
        assert offset >= end, "spans overlap"
        if route == RING:
            assert room(span, p) == 0 and offset == end  # takes no bounce bytes
        elif route == IN_PLACE:
            assert may
            assert pitch == up(width, 16) and rows * pitch < STAGE
        else:
            assert pitch == width and rows * width < STAGE
        assert offset == end  # packed in the order given
        end = offset + room(span, p)
    assert total == end, "the total is the end of the last span"
    return placed, total


PINNED = [
    ((1, 4, True), IN_PLACE),
    ((3, 28, True), IN_PLACE),
    ((3, 11184804, True), BOUNCE),   # flm_prg_expand K = 3, L = 2796201: packed under 32 MiB, padded not
    ((2, 16777212, True), BOUNCE),
    ((2, 16777216, True), RING),
    ((1, 33554431, True), BOUNCE),
    ((1, 33554432, False), RING),
]


@pytest.mark.parametrize("span,route", PINNED)
def test_pinned_routes(span, route):
    placed, total = check_properties([span])
    assert placed[0][0] == route
    rows, width, _ = span
    if route == BOUNCE:
        assert total >= rows * width
    # the same span keeps its route and its room among others, whatever comes before it
    placed3, total3 = check_properties([(2, 100, False), span, (1, 7, True)])
    assert placed3[1][:2] == placed[0][:2]
    assert total3 == up(200, 256) + total + 256


def test_the_expand_gap_reserves_what_its_dma_copies():
    """K = 3, L = 2796201 words: the packed plane is 33,554,412 B (under 32 MiB), the in-place plane
    at a 16-byte pitch 33,554,448 B (not under it).  The span goes through the bounce buffer by DMA
    and the layout reserves at least the bytes that DMA copies."""
    placed, total = check_properties([(3, 32, False), (3, 11184804, True)])
    assert 3 * 11184804 == 33554412 and 3 * up(11184804, 16) == 33554448
    assert placed[1][0] == BOUNCE and placed[1][1] == 11184804
    assert total - placed[1][2] >= 33554412


@pytest.mark.parametrize("c1,points,seeds", list(itertools.product((False, True), repeat=3)))
def test_ec_combine_spans_present_or_absent(c1, points, seeds):
    """flm_ec_combine at T = 20, D = 1000: shares, lambdas, [c1], flags, [points_out], [seeds_out]."""
    T, D = 20, 1000
    spans = [(1, T * D * 64, False), (1, T * 32, False)]
    spans += [(1, D * 64, False)] if c1 else []
    spans += [(1, D * 4, False)]
    spans += [(1, D * 64, False)] if points else []
    spans += [(1, D * 32, False)] if seeds else []
    placed, total = check_properties(spans)
    assert all(p[0] == BOUNCE for p in placed)
    assert total == sum(up(rows * width, 256) for rows, width, _ in spans)


def test_properties_over_mixed_calls():
    g = np.random.Generator(np.random.PCG64(5))
    edges = [0, 1, 15, 16, 17, 255, 256, 257, 4096, STAGE // 2 - 1, STAGE // 2, STAGE - 16, STAGE - 15, STAGE - 1,
             STAGE, STAGE + 1]
    for _ in range(300):
        spans = []
        for _ in range(int(g.integers(0, 7))):
            width = int(g.choice(edges)) if g.random() < 0.7 else int(g.integers(1, 1 << 22))
            rows = int(g.choice([0, 1, 2, 3, 9, 1000]))
            spans.append((rows, width, bool(g.integers(0, 2))))
        check_properties(spans)
    assert layout([]) == ([], 0)
