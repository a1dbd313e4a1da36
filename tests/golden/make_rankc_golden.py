#!/usr/bin/env python3
"""Generate tests/golden/rankc_ref.json from the REFERENCE ITSELF (BitMagic 9.2.1 compiled by oracle/Makefile into oracle/_ref/).
The reference shim exports no rank_compressor, so the generator applies the reference's own per-bit rule through the calls
that exist (rankc_cases.py): compress sets bit count_to(p) - 1 for every one p of src & idx on an empty reference vector (the
body of compress_by_source's visitor, src/bmalgo.h:673-674); decompress sets bit select(s + 1) for every one s of src (what
decompress reaches through find_rank, :593-612).  Then flatten, optimize(), flatten again.  Per case and direction the fixture
keeps the size, the count, record() of both tables and a hash of the positions of the ones: hashes, not bit data.  Index blocks
at or beyond 2^32 go through the 48-bit address build (avx2_64).

    python tests/golden/make_rankc_golden.py            # writes rankc_ref.json
    python tests/golden/make_rankc_golden.py --check    # regenerates in memory and compares with the committed file
"""
from __future__ import annotations

import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, HERE)

import oracle  # noqa: E402
from rankc_cases import cases, oracle_case  # noqa: E402

OUT = os.path.join(HERE, "rankc_ref.json")


def generate() -> str:
    out = {"reference": None, "cases": {}}
    for name, case in cases().items():
        R = oracle.reference(case["flavour"])
        out["reference"] = R.name if case["flavour"] == "avx2" else out["reference"]
        out["cases"][name] = oracle_case(R, name, case)
    return json.dumps(out, indent=1, sort_keys=True) + "\n"


if __name__ == "__main__":
    txt = generate()
    if "--check" in sys.argv:
        same = open(OUT).read() == txt
        print("rankc_ref.json reproduced" if same else "rankc_ref.json DIFFERS")
        sys.exit(0 if same else 1)
    with open(OUT, "w") as f:
        f.write(txt)
    print("wrote", OUT, len(txt), "bytes")
