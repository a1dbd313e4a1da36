#!/usr/bin/env python3
"""Generate tests/golden/pair_ref.json from the REFERENCE ITSELF (BitMagic 9.2.1 compiled by oracle/Makefile into oracle/_ref/):
bit_and / bit_or / bit_xor / bit_sub of the constructed case pairs of pair_cases.py -- the short form in all four import
flavours, the partial-block pair, the long form at 2,049 blocks and the one-level chain -- under opt_none and opt_compress.
Everything is built by import_words and op2.  Per result the fixture keeps the block kinds (two blocks per hexadecimal digit,
pair_cases.kinds_str), the count and a SHA-256 of the words, per operand its kinds: hashes, no bit data.

    python tests/golden/make_pair_golden.py            # writes pair_ref.json
    python tests/golden/make_pair_golden.py --check    # regenerates in memory and compares with the committed file
"""
from __future__ import annotations

import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, HERE)

import oracle  # noqa: E402
from pair_cases import oracle_fixture  # noqa: E402

OUT = os.path.join(HERE, "pair_ref.json")


def generate() -> str:
    R = oracle.reference("avx2")
    out = {"reference": R.name}
    out.update(oracle_fixture(R))
    return json.dumps(out, indent=0, sort_keys=True) + "\n"


if __name__ == "__main__":
    txt = generate()
    if "--check" in sys.argv:
        same = open(OUT).read() == txt
        print("pair_ref.json reproduced" if same else "pair_ref.json DIFFERS")
        sys.exit(0 if same else 1)
    with open(OUT, "w") as f:
        f.write(txt)
    print("wrote", OUT, len(txt), "bytes")
