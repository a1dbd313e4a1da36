#!/usr/bin/env python3
"""Which rows differ between two resident columns in ONE pass (bmx_slice_mismatch / bmx_slice_first_mismatch, DESIGN_KERNELS.md 2.23)
against the composition of whole-vector calls it replaces and leaves unchanged: P x bmx_op2(XOR) with every temporary alive, one
bmx_agg_or over them, then the NULL passes.  Both routes run in the same process, alternating, on the same operands, and must give
identical results.

Operands (all from seeds): 32 planes x 1e9 rows at 50 %; column b = column a with 0.1 % of the rows changed (a change mask at
0.1 %, and per plane a random half of it inverted); not-NULL vectors at 95 % that differ in 0.01 % of the rows.  Column c holds a's
content under handles of its own (equal planes given as the SAME handles are skipped without a read).

Cases, one JSON line each:
  vector_use_null / vector_no_null   the mismatch vector            a against b
  count_use_null                     its population count only      a against b
  first_early                        the first mismatch             a against b (a hit in the first block column)
  first_absent                       the first mismatch             a against c (every plane block of both columns is read)

ms = host clock around the call (both routes end in a device synchronise), median of --runs after --warmup calls of each route, with
min / max = the run-to-run spread; read_bytes / write_bytes = the ALGORITHMIC bytes of the fused call (every plane and not-NULL
block once, plus the result's blocks); hbm_fraction = those bytes over the fused call's time over the 8.0 TB/s HBM peak.

    python tools/bench_sv_mismatch.py [--cases vector_use_null,...] [--planes 32] [--nbits 1000000000] [--runs 7] [--warmup 2]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

import bitmagic_amd as bm  # noqa: E402

SEED = 0xB17A61C
HBM_PEAK = 8.0e12
CASES = ("vector_use_null", "vector_no_null", "count_use_null", "first_early", "first_absent")


def build(ctx, planes: int, nbits: int):
    a = [bm.bvector.generate(ctx, SEED, 500 + i, 32768, nbits) for i in range(planes)]
    change = bm.bvector.generate(ctx, SEED, 900, 66, nbits)                           # 0.1 % of the rows
    b, c = [], []
    for i in range(planes):
        half = bm.bvector.generate(ctx, SEED, 600 + i, 32768, nbits)
        b.append(bm.bvector.bit_xor(a[i], bm.bvector.bit_and(change, half)))
        c.append(bm.bvector.bit_and(a[i], a[i]))
    na = bm.bvector.generate(ctx, SEED, 901, 62259, nbits)                             # 95 % not NULL
    nb = bm.bvector.bit_xor(na, bm.bvector.generate(ctx, SEED, 902, 7, nbits))
    nc = bm.bvector.bit_and(na, na)
    mk = lambda p, n: bm.slice_scanner(ctx, p, size=nbits, not_null=n)
    return mk(a, na), mk(b, nb), mk(c, nc)


def composed_vector(ctx, x, y, proc):
    """P x op2(XOR), every temporary alive; agg_or over them; the NULL passes (equal sizes: no size term)"""
    tmp = [bm.bvector.bit_xor(p, q) for p, q in zip(x.slices, y.slices)]
    d = bm.aggregator(ctx).combine_or(tmp)
    if proc == bm.USE_NULL:
        return bm.bvector.bit_or(d, bm.bvector.bit_xor(x.not_null, y.not_null))
    return bm.bvector.bit_and(d, bm.bvector.bit_or(x.not_null, y.not_null))


def routes(ctx, case, a, b, c):
    """-> (fused, composed, same): two callables and the comparison of their results"""
    if case.startswith("vector"):
        proc = bm.USE_NULL if case.endswith("use_null") else bm.NO_NULL
        same = lambda n, o: n.size() == o.size() and n.count() == o.count() and bm.count_xor(n, o) == 0
        return (lambda: bm.sparse_vector_find_mismatch(a, b, proc)), (lambda: composed_vector(ctx, a, b, proc)), same
    if case == "count_use_null":
        return (lambda: bm.sparse_vector_count_mismatch(a, b, bm.USE_NULL)), (lambda: composed_vector(ctx, a, b, bm.USE_NULL).count()), lambda n, o: n == o
    y = b if case == "first_early" else c
    # (equal sizes and both not-NULL vectors: F of the first mismatch is the use_null vector)
    return (lambda: bm.sparse_vector_find_first_mismatch(a, y, bm.USE_NULL)), (lambda: composed_vector(ctx, a, y, bm.USE_NULL).find()), \
        lambda n, o: bool(n[0]) == bool(o[0]) and (not n[0] or int(n[1]) == int(o[1]))


def timed(fn, ctx):
    ctx.synchronize()
    t0 = time.perf_counter()
    out = fn()
    ctx.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def stats(ts):
    return {"ms": round(float(np.median(ts)), 3), "min": round(min(ts), 3), "max": round(max(ts), 3), "runs": len(ts)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--planes", type=int, default=32)
    ap.add_argument("--nbits", type=int, default=1_000_000_000)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    ctx = bm.context(0)
    a, b, c = build(ctx, args.planes, args.nbits)
    col_bytes = lambda s: sum(p.operand_bytes() for p in s.slices) + s.not_null.operand_bytes()
    for case in args.cases.split(","):
        fused, composed, same = routes(ctx, case, a, b, c)
        y = c if case == "first_absent" else b
        rec = {"case": case, "planes": args.planes, "rows": args.nbits, "read_bytes": col_bytes(a) + col_bytes(y), "write_bytes": 0}
        for _ in range(args.warmup):
            new = fused(); old = composed()
        rec["identical"] = bool(same(new, old))
        if case.startswith("vector"):
            i = new.info()
            rec["write_bytes"] = i["counts"][bm.BIT] * 8192 + i["gap_words"] * 2
            rec["result_count"] = new.count()
        else:
            rec["result"] = [int(x) for x in new] if isinstance(new, tuple) else int(new)
        del new, old
        tn, to = [], []
        for _ in range(args.runs):                                              # alternating
            t, r = timed(fused, ctx); tn.append(t); del r
            t, r = timed(composed, ctx); to.append(t); del r
        rec["fused"] = stats(tn); rec["composed"] = stats(to)
        rec["speedup"] = round(rec["composed"]["ms"] / rec["fused"]["ms"], 2)
        rec["faster_beyond_spread"] = bool(rec["fused"]["max"] < rec["composed"]["min"])
        if case != "first_early":                                               # (an early hit reads one window, not the columns)
            rec["hbm_fraction"] = round((rec["read_bytes"] + rec["write_bytes"]) / (rec["fused"]["ms"] * 1e-3) / HBM_PEAK, 3)
        print(json.dumps(rec), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
