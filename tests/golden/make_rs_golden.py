#!/usr/bin/env python3
"""Generate tests/golden/rs_ref.json from the REFERENCE ITSELF (BitMagic 9.2.1 compiled by oracle/Makefile into oracle/_ref/):
rs_index and count_to / select over the constructed cases of rs_cases.py that fit a 32-bit vector.  Per case the fixture keeps
the count, a SHA-256 of the exported bcount / sub_count, a SHA-256 of the rank answers and of the select answers over the
case's query lists (positions and ranks below 2^32 - 1), a dozen literal values, and for grid A count_range, rank_corrected,
count_to_test and find_rank over its constructed list: hashes, no bit data.

    python tests/golden/make_rs_golden.py            # writes rs_ref.json
    python tests/golden/make_rs_golden.py --check    # regenerates in memory and compares with the committed file
"""
from __future__ import annotations

import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, HERE)

import oracle  # noqa: E402
from rs_cases import oracle_fixture  # noqa: E402

OUT = os.path.join(HERE, "rs_ref.json")


def generate() -> str:
    R = oracle.reference("avx2")
    out = {"reference": R.name}
    out.update(oracle_fixture(R))
    return json.dumps(out, indent=0, sort_keys=True) + "\n"


if __name__ == "__main__":
    txt = generate()
    if "--check" in sys.argv:
        same = open(OUT).read() == txt
        print("rs_ref.json reproduced" if same else "rs_ref.json DIFFERS")
        sys.exit(0 if same else 1)
    with open(OUT, "w") as f:
        f.write(txt)
    print("wrote", OUT, len(txt), "bytes")
