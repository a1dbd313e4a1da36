#!/usr/bin/env python3
"""Generate tests/golden/remap_ref.json: what bm::set2set_11_transform<SV>::remap (src/bmsparsevec_algo.h:2096-2205) gives for the
cases of remap_cases.py -- per case the number of translated rows, hashes of the row ids and of the values in row order, and the
count, hash and largest element of the image: hashes, counts and sizes, no bit data.

The numbers come from the NumPy model of remap_cases.py.  The reference shim exports no set2set, so every case that can be
(built from values, unsigned, at most 32 planes, at most a few hundred distinct image values) is anchored in the REFERENCE ITSELF
(BitMagic 9.2.1 compiled by oracle/Makefile into oracle/_ref/) before its record is written (remap_cases.anchor_case): the planes
and the not-NULL vector are the slices of a bm::sparse_vector<> built from the same values, every image value is found by
sparse_vector_scanner::find_eq among the selected rows, and those per-value counts add up to count(sel & not_null).

    python tests/golden/make_remap_golden.py            # writes remap_ref.json
    python tests/golden/make_remap_golden.py --check    # regenerates in memory and compares with the committed file
"""
from __future__ import annotations

import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, HERE)

import oracle  # noqa: E402
from remap_cases import anchor_case, anchored, cases, model_case, record  # noqa: E402

OUT = os.path.join(HERE, "remap_ref.json")


def generate() -> str:
    R = oracle.reference("avx2")
    out = {"reference": R.name, "cases": {}}
    for name, case in cases().items():
        r = record(model_case(case))
        r["anchored"] = anchor_case(R, case) if anchored(case) else None
        out["cases"][name] = r
    return json.dumps(out, indent=1, sort_keys=True) + "\n"


if __name__ == "__main__":
    txt = generate()
    if "--check" in sys.argv:
        same = open(OUT).read() == txt
        print("remap_ref.json reproduced" if same else "remap_ref.json DIFFERS")
        sys.exit(0 if same else 1)
    with open(OUT, "w") as f:
        f.write(txt)
    print("wrote", OUT, len(txt), "bytes")
