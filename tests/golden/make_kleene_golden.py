#!/usr/bin/env python3
"""Generate tests/golden/kleene_ref.json from the REFERENCE ITSELF (BitMagic 9.2.1 compiled by oracle/Makefile into oracle/_ref/).
The reference shim exports no three-valued logic, so the generator applies the reference's own sequences -- or_kleene
(src/bm3vl.h:186-197) and and_kleene (:250-261) -- through Oracle.op2 of the reference build, which is every call those functions
make (kleene_cases.py).  A list of pairs is folded from the left with the in-place form; then optimize() and flatten.  Per case,
operation and output the fixture keeps the size, the count, record() of the optimised table and a hash of the positions of the
ones, and per case and operation the three counts (false, unknown, true): hashes, not bit data.

    python tests/golden/make_kleene_golden.py            # writes kleene_ref.json
    python tests/golden/make_kleene_golden.py --check    # regenerates in memory and compares with the committed file
"""
from __future__ import annotations

import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, HERE)

import oracle  # noqa: E402
from kleene_cases import cases, oracle_case  # noqa: E402

OUT = os.path.join(HERE, "kleene_ref.json")


def generate() -> str:
    R = oracle.reference("avx2")
    out = {"reference": R.name, "cases": {name: oracle_case(R, case) for name, case in cases().items()}}
    return json.dumps(out, indent=1, sort_keys=True) + "\n"


if __name__ == "__main__":
    txt = generate()
    if "--check" in sys.argv:
        same = open(OUT).read() == txt
        print("kleene_ref.json reproduced" if same else "kleene_ref.json DIFFERS")
        sys.exit(0 if same else 1)
    with open(OUT, "w") as f:
        f.write(txt)
    print("wrote", OUT, len(txt), "bytes")
