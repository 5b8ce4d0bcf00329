"""The caller's side of the decode modulo the field (include/flamingo_hip.h): host Python, stdlib
only.  The library follows carries between the packed fields and reports how close the centred sums came to the
half-modulus H = 2^(32/pack - 1); it bounds nothing about the probability of a wrap.  This module turns the caller's
choices into the library's arguments and the library's report into a distance.

* half_modulus(pack): H.
* guard(pack, fraction): ceil(fraction * H) clamped to 1..H, the integer guard of MaskEngine.decode_unpack_mod.
* margin_sigmas(pack, count, signal_bound, share_var): (H - signal_bound) / sqrt(count * share_var): how many standard
  deviations of the summed noise lie between the largest signal sum the caller expects and the wrap.  share_var is the
  variance of one client's share: noise_bits / 4 for the binomial share, dgauss.moments(table)[1] for the table mode.
  A distance in noise standard deviations, labelled as such: no probability, and no (epsilon, delta).
"""
from __future__ import annotations

import math
from fractions import Fraction


def half_modulus(pack: int) -> int:
    """H = 2^(32/pack - 1) for pack 2 or 4: the centred sums lie in [-H, H - 1]."""
    if pack not in (2, 4):
        raise ValueError("pack must be 2 or 4")
    return 1 << (32 // pack - 1)


def guard(pack: int, fraction: float) -> int:
    """ceil(fraction * H), clamped to 1..H; fraction a finite number (the agents pass one in (0, 1])."""
    H = half_modulus(pack)
    f = float(fraction)
    if not math.isfinite(f):
        raise ValueError("fraction must be finite")
    return min(H, max(1, math.ceil(Fraction(f) * H)))


def margin_sigmas(pack: int, count: int, signal_bound: float, share_var) -> float:
    """(H - signal_bound) / sqrt(count * share_var), in standard deviations of the summed noise; inf without noise
    (share_var = 0) when the signal stays below H, -inf when it does not.  Not a probability."""
    H = half_modulus(pack)
    if int(count) != count or count < 1:
        raise ValueError("count must be an integer >= 1")
    var = float(share_var)
    if not (var >= 0.0) or not math.isfinite(var):
        raise ValueError("share_var must be finite and not negative")
    room = float(H) - float(signal_bound)
    if var == 0.0:
        return math.inf if room > 0.0 else -math.inf if room < 0.0 else 0.0
    return room / math.sqrt(int(count) * var)
