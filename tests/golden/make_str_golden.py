#!/usr/bin/env python3
"""Generate tests/golden/str_ref.json: what a string search over the planes of a bm::str_sparse_vector<> gives for the cases of
str_cases.py (find_eq_str and its batch forms, src/bmsparsevec_algo.h:1194-1235, 2546-2588, 3263-3436) -- per case the number of
keys, the total of their counts, hashes of the counts, of the first rows and of the index lists, and the AND / SUB plane lists of
its first single searches: hashes, counts and plane numbers, no bit data.

The numbers come from the NumPy model of str_cases.py (byte-wise row equality).  The reference shim exports no string container, so
every case is anchored in the REFERENCE ITSELF (BitMagic 9.2.1 compiled by oracle/Makefile into oracle/_ref/) before its record is
written (str_cases.anchor_case): reference vectors are built from the same planes, and the AND-SUB groups of the case's first 200
distinct keys run through the reference's counts pipeline and find_first_and_sub; model and reference must agree.

    python tests/golden/make_str_golden.py            # writes str_ref.json
    python tests/golden/make_str_golden.py --check    # regenerates in memory and compares with the committed file
"""
from __future__ import annotations

import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, HERE)

import oracle  # noqa: E402
from bitmagic_amd import str_search_groups  # noqa: E402
from str_cases import anchor_case, cases, model_case, record  # noqa: E402

OUT = os.path.join(HERE, "str_ref.json")


def generate() -> str:
    R = oracle.reference("avx2")
    out = {"reference": R.name, "cases": {}}
    for name, case in cases().items():
        m = model_case(case)
        r = record(case, m, str_search_groups)
        r["anchored"] = anchor_case(R, case, m, str_search_groups)
        out["cases"][name] = r
    return json.dumps(out, indent=1, sort_keys=True) + "\n"


if __name__ == "__main__":
    txt = generate()
    if "--check" in sys.argv:
        same = open(OUT).read() == txt
        print("str_ref.json reproduced" if same else "str_ref.json DIFFERS")
        sys.exit(0 if same else 1)
    with open(OUT, "w") as f:
        f.write(txt)
    print("wrote", OUT, len(txt), "bytes")
