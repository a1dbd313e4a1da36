#!/usr/bin/env python3
"""Generate tests/golden/or_ref.json from the REFERENCE ITSELF (BitMagic 9.2.1 compiled by oracle/Makefile into oracle/_ref/):
aggregator::combine_or over a fixed subset of the constructed lists of or_cases.py (every fourth case of grid O1, every sixth
of O2) and over the full member list of every O3 / O5 collection, under opt_none and opt_compress.  The operands are imported
from their bits.  Per result the fixture keeps the block kinds (a digit per block), the count and a SHA-256 of the words:
hashes, no bit data.

    python tests/golden/make_or_golden.py            # writes or_ref.json
    python tests/golden/make_or_golden.py --check    # regenerates in memory and compares with the committed file
"""
from __future__ import annotations

import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, HERE)

import oracle  # noqa: E402
from or_cases import oracle_fixture  # noqa: E402

OUT = os.path.join(HERE, "or_ref.json")


def generate() -> str:
    R = oracle.reference("avx2")
    out = {"reference": R.name}
    out.update(oracle_fixture(R))
    return json.dumps(out, indent=0, sort_keys=True) + "\n"


if __name__ == "__main__":
    txt = generate()
    if "--check" in sys.argv:
        same = open(OUT).read() == txt
        print("or_ref.json reproduced" if same else "or_ref.json DIFFERS")
        sys.exit(0 if same else 1)
    with open(OUT, "w") as f:
        f.write(txt)
    print("wrote", OUT, len(txt), "bytes")
