#!/usr/bin/env python3
"""Generate tests/golden/range_ref.json from the REFERENCE ITSELF (BitMagic 9.2.1 compiled by oracle/Makefile into oracle/_ref/):
for the pair lists of range_cases.py, bvector::set_range(l, r) per pair on an empty vector (src/bm.h:2398), optimize(opt_compress),
then the optimised block table and the maximal runs of ones of the reference's own words (what a bm::interval_enumerator loop
yields, src/bmintervals.h:52-226).  Ends at or beyond 2^32 go through the 48-bit address build (avx2_64).

    python tests/golden/make_range_golden.py            # writes range_ref.json
    python tests/golden/make_range_golden.py --check    # regenerates in memory and compares with the committed file
"""
from __future__ import annotations

import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, HERE)

import oracle  # noqa: E402
from range_cases import cases, oracle_table, record, sha  # noqa: E402

OUT = os.path.join(HERE, "range_ref.json")


def case_record(o, pairs, nbits) -> dict:
    nbits_out, table, count, runs = oracle_table(o, pairs, nbits)
    return {"nbits_out": nbits_out, "count": count, "table": record(*table), "intervals": int(runs.shape[0]),
            "intervals_sha": sha(runs.astype("<u8"))}


def generate() -> str:
    out = {"reference": None, "cases": {}}
    for name, (pairs, nbits, flavour) in cases().items():
        R = oracle.reference(flavour)
        out["reference"] = R.name if flavour == "avx2" else out["reference"]
        c = {"flavour": flavour, "nbits": int(nbits), "n": int(pairs.shape[0])}
        c.update(case_record(R, pairs, nbits))
        out["cases"][name] = c
    return json.dumps(out, indent=1, sort_keys=True) + "\n"


if __name__ == "__main__":
    txt = generate()
    if "--check" in sys.argv:
        same = open(OUT).read() == txt
        print("range_ref.json reproduced" if same else "range_ref.json DIFFERS")
        sys.exit(0 if same else 1)
    with open(OUT, "w") as f:
        f.write(txt)
    print("wrote", OUT, len(txt), "bytes")
