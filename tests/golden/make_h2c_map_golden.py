"""Golden map_to_curve points produced BY THE REFERENCE'S OWN CODE (build container only).

Imports util/crypto/ecchash.py read-only from /root/reference under tests/golden/refshim.py (as
make_h2c_golden.py does) and calls its own ecchash.map_to_curve(u) on every u of the map family of
tests/h2c_cases.py: the edge inputs that no message reaches, which hash_str_to_curve's table
(h2c_golden.json) therefore cannot pin.  Records (tests/golden/h2c_map_golden.json):
  * points: u, x, y (hex) for every u whose denominator 100 u^4 - 10 u^2 is not 0 mod p;
  * raises: the three u at which it is 0 -- u = 0 and both square roots of 1/10 -- where the
    reference has no answer: libnum.invmod(0, p) raises (refshim's stand-in is pow(0, -1, p), which
    raises ValueError; libnum's own raises too), so the `tv1 == 0` branch of ecchash.py:247-248 is
    dead code.  The kernel and oracle/ec_oracle.py take RFC 9380's inv0 there.
The square-root order is refshim's assumption, as in h2c_golden.json ("parity unpinned").

Reproduce:  python tests/golden/make_h2c_map_golden.py            (writes the file)
            python tests/golden/make_h2c_map_golden.py --print    (prints it instead)
"""
from __future__ import annotations

import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
P = 2**256 - 2**224 + 2**192 + 2**96 - 1


def _setup():
    sys.path.insert(0, HERE)
    import refshim
    refshim.install()
    sys.path.insert(0, REF)
    from util.crypto import ecchash
    return ecchash


def generate() -> dict:
    ecchash = _setup()
    sys.path.insert(0, os.path.dirname(HERE))
    import h2c_cases as C
    points, raises, seen = [], [], set()
    for name, v in C.map_values():
        u = v % ecchash.n
        if u in seen:                      # the other spellings of 0
            continue
        seen.add(u)
        try:
            pt = ecchash.map_to_curve(u)
        except Exception as e:              # noqa: BLE001 -- whatever the reference's invmod raises
            raises.append({"name": name, "u": f"{u:064x}", "error": type(e).__name__})
            continue
        points.append({"name": name, "u": f"{u:064x}", "x": f"{int(pt.x) % P:064x}", "y": f"{int(pt.y) % P:064x}"})
    return {"what": "ecchash.map_to_curve(u) by the reference's own util/crypto/ecchash.py (refshim stand-ins for "
                    "pycryptodomex/libnum) on the map family of tests/h2c_cases.py",
            "parity": "parity unpinned: libnum's sqrtmod root order (ecchash.py:263-268), as in h2c_golden.json",
            "inv0": "at the u under 'raises' the denominator is 0 and the reference's libnum.invmod raises: "
                    "ecchash.py:247-248 is dead code; this project takes RFC 9380's inv0 (0 -> 0) there",
            "points": points, "raises": raises}


if __name__ == "__main__":
    rec = generate()
    text = json.dumps(rec, indent=0, sort_keys=True)
    if "--print" in sys.argv:
        print(text)
    else:
        with open(os.path.join(HERE, "h2c_map_golden.json"), "w") as f:
            f.write(text + "\n")
        print(len(rec["points"]), "points,", len(rec["raises"]), "u at which the reference raises")
