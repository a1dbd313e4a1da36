#!/usr/bin/env python3
"""Generate tests/golden/sv_mismatch_ref.json from the REFERENCE ITSELF (BitMagic 9.2.1 compiled by oracle/Makefile into
oracle/_ref/).  The reference shim exports neither sparse_vector_find_mismatch nor sparse_vector_find_first_mismatch, so the
generator replays the reference's own sequences of whole-vector calls (src/bmsparsevec_algo.h:656-792 and :478-636) through
Oracle.op2, Vec.set_range and Oracle.find_first of the reference build (sv_mismatch_cases.py).  Per case and null_proc the fixture
keeps the result's size, the count, a hash of the positions of the ones and (found, idx) of the first mismatch: hashes, no bit data.
The planes of the value-column case are also compared with the slices of a bm::sparse_vector<> built from the same values.

    python tests/golden/make_sv_mismatch_golden.py            # writes sv_mismatch_ref.json
    python tests/golden/make_sv_mismatch_golden.py --check    # regenerates in memory and compares with the committed file
"""
from __future__ import annotations

import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, HERE)

import oracle  # noqa: E402
from sv_mismatch_cases import cases, ones_of, oracle_case  # noqa: E402

OUT = os.path.join(HERE, "sv_mismatch_ref.json")


def check_value_planes(R) -> None:
    """the bit-sliced planes of the value columns are the slices the reference's container holds"""
    case = cases()["values_32"]
    va, vb, null_a, null_b = case["values"]
    for side, v, nl in (("a", va, null_a), ("b", vb, null_b)):
        sv = R.sparse_vector(v, nl.astype(np.uint8))
        assert sv.size() == v.size
        for i in range(32):
            s = sv.slice(i)
            got = ones_of(s) if s is not None else np.zeros(0, np.uint64)
            assert np.array_equal(got, case["vecs"]["%s%d" % (side, i)][0]), (side, i)
        assert np.array_equal(ones_of(sv.not_null()), case["vecs"]["n" + side][0]), side


def generate() -> str:
    R = oracle.reference("avx2")
    check_value_planes(R)
    out = {"reference": R.name, "cases": {name: oracle_case(R, case) for name, case in cases().items()}}
    return json.dumps(out, indent=1, sort_keys=True) + "\n"


if __name__ == "__main__":
    txt = generate()
    if "--check" in sys.argv:
        same = open(OUT).read() == txt
        print("sv_mismatch_ref.json reproduced" if same else "sv_mismatch_ref.json DIFFERS")
        sys.exit(0 if same else 1)
    with open(OUT, "w") as f:
        f.write(txt)
    print("wrote", OUT, len(txt), "bytes")
