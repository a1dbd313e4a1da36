#!/usr/bin/env python3
"""Generate tests/golden/ids_ref.json from the REFERENCE ITSELF (BitMagic 9.2.1 compiled by oracle/Makefile into oracle/_ref/):
the block tables of the recorded subset of ids_cases.py (ids_cases.recorded(): the GAP level and threshold cases of I3, all of
I6, every fourth case of I1 and I4), without and with optimize().  The reference is driven the way import_cases.oracle_table
drives it -- set_bit per id, then optimize() -- because its import_sorted(..., true) leaves the list's last block unoptimised
(DESIGN_KERNELS.md 2.19).  Ids at or beyond 2^32 go through the 48-bit address build (avx2_64).

    python tests/golden/make_ids_golden.py            # writes ids_ref.json
    python tests/golden/make_ids_golden.py --check    # regenerates in memory and compares with the committed file
"""
from __future__ import annotations

import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, HERE)

import oracle  # noqa: E402
from ids_cases import recorded  # noqa: E402
from import_cases import oracle_table, record  # noqa: E402

OUT = os.path.join(HERE, "ids_ref.json")


def generate() -> str:
    out = {"reference": oracle.reference("avx2").name, "cases": {}}
    for case in recorded():
        R = oracle.reference(case.flavour)
        ids = case.ids()
        c = {"flavour": case.flavour, "nbits": case.nbits, "n": int(ids.size)}
        for opt in (0, 1):
            nbits_out, table, count = oracle_table(R, ids, case.nbits, bool(opt))
            c["nbits_out"] = nbits_out
            c["count"] = count
            c[f"opt{opt}"] = record(*table)
        out["cases"][case.name] = c
    return json.dumps(out, indent=1, sort_keys=True) + "\n"


if __name__ == "__main__":
    txt = generate()
    if "--check" in sys.argv:
        same = open(OUT).read() == txt
        print("ids_ref.json reproduced" if same else "ids_ref.json DIFFERS")
        sys.exit(0 if same else 1)
    with open(OUT, "w") as f:
        f.write(txt)
    print("wrote", OUT, len(txt), "bytes")
