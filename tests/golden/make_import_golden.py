#!/usr/bin/env python3
"""Generate tests/golden/import_ref.json from the REFERENCE ITSELF (BitMagic 9.2.1 compiled by oracle/Makefile into
oracle/_ref/): the block tables of bvector::set(ids, n, sort_order) on an empty vector (src/bm.h:4153) for the id lists of
import_cases.py, without and with optimize().  Ids at or beyond 2^32 go through the 48-bit address build (avx2_64).

    python tests/golden/make_import_golden.py            # writes import_ref.json
    python tests/golden/make_import_golden.py --check    # regenerates in memory and compares with the committed file
"""
from __future__ import annotations

import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, HERE)

import oracle  # noqa: E402
from import_cases import cases, oracle_table, record  # noqa: E402

OUT = os.path.join(HERE, "import_ref.json")


def generate() -> str:
    out = {"reference": None, "cases": {}}
    for name, (ids, nbits, flavour) in cases().items():
        R = oracle.reference(flavour)
        out["reference"] = R.name if flavour == "avx2" else out["reference"]
        c = {"flavour": flavour, "nbits": int(nbits), "n": int(ids.size)}
        for opt in (0, 1):
            nbits_out, table, count = oracle_table(R, ids, nbits, bool(opt))
            c["nbits_out"] = nbits_out
            c["count"] = count
            c[f"opt{opt}"] = record(*table)
        out["cases"][name] = c
    return json.dumps(out, indent=1, sort_keys=True) + "\n"


if __name__ == "__main__":
    txt = generate()
    if "--check" in sys.argv:
        same = open(OUT).read() == txt
        print("import_ref.json reproduced" if same else "import_ref.json DIFFERS")
        sys.exit(0 if same else 1)
    with open(OUT, "w") as f:
        f.write(txt)
    print("wrote", OUT, len(txt), "bytes")
