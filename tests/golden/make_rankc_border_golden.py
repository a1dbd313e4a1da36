#!/usr/bin/env python3
"""Generate tests/golden/rankc_border_ref.json from the REFERENCE ITSELF (BitMagic 9.2.1 compiled by oracle/Makefile into
oracle/_ref/), by the method of make_rankc_golden.py: the reference shim exports no rank_compressor, so the reference's own per-bit
rule goes through the calls that exist (rankc_border_cases.oracle_record): compress sets bit count_to(p) - 1 for every one p of
src & idx on an empty reference vector, decompress sets bit select(s + 1) for every one s of src; then flatten, optimize(), flatten
again.  Recorded (rankc_border_cases.RECORDED): all of grid W, the D and E cases that name a shortcut, a tie or a split word
(D/kinds, E/split, E/ties), and the case past 2^32 with its sparse index-space source (48-bit address build, avx2_64; its index is
set_range over the 65,536 FULL blocks plus set_bit for the tail).  Per case, source and direction the fixture keeps the size, the
count, record() of both tables and a hash of the positions: hashes, not bit data.

    python tests/golden/make_rankc_border_golden.py            # writes rankc_border_ref.json
    python tests/golden/make_rankc_border_golden.py --check    # regenerates in memory and compares with the committed file
"""
from __future__ import annotations

import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, HERE)

import oracle  # noqa: E402
import rankc_border_cases as rb  # noqa: E402

OUT = os.path.join(HERE, "rankc_border_ref.json")


def generate() -> str:
    out = {"reference": None, "cases": {}}
    for case, sname in rb.recorded():
        R = oracle.reference(case.flavour)
        out["reference"] = R.name if case.flavour == "avx2" else out["reference"]
        c = out["cases"].setdefault(case.name, {"flavour": case.flavour, "idx_count": case.idx.count, "idx_nbits": case.idx.nbits,
                                                "sources": {}})
        c["sources"][sname] = {d: rb.oracle_record(R, case, sname, d) for d in rb.DIRECTIONS}
    lines = ['{"reference": %s, "cases": {' % json.dumps(out["reference"])]
    names = sorted(out["cases"])
    for i, n in enumerate(names):                              # one line per case keeps the file small and the diffs readable
        lines.append("%s: %s%s" % (json.dumps(n), json.dumps(out["cases"][n], sort_keys=True, separators=(",", ":")),
                                   "," if i + 1 < len(names) else ""))
    lines.append("}}")
    return "\n".join(lines) + "\n"


if __name__ == "__main__":
    txt = generate()
    if "--check" in sys.argv:
        same = open(OUT).read() == txt
        print("rankc_border_ref.json reproduced" if same else "rankc_border_ref.json DIFFERS")
        sys.exit(0 if same else 1)
    with open(OUT, "w") as f:
        f.write(txt)
    print("wrote", OUT, len(txt), "bytes")
