#!/usr/bin/env python3
"""Every arg-group's hits as one CSR (bmx_pipeline_run_indices, DESIGN_KERNELS.md 2.22) against the route that existed before it:
bmx_pipeline_run_results plus one bmx_vec_to_indices per non-NULL result.  Both routes run in the same process, alternating, on
the same pipeline, and must produce identical arrays.

Shapes (all from seeds):
  scanner  2,048 equality groups over 32 planes x 1e9 rows at 50 % (one AND-SUB group per value, tools/bench_scanner.py)
  and8     256 groups of 8 AND + 2 SUB operands drawn from 64 vectors of 1e9 bits at 1 % (AND material shares the generator's
           common bits, so the groups have hits)

One JSON line per shape: ms = host clock around the call (both routes end in a device synchronise), median of --runs after
--warmup, with min / max; operand_bytes = the algorithmic operand bytes of one pass over the pipeline (bmx_pipeline_operand_bytes;
the new route makes at most two passes, the second only over items with hits); table_bytes = the (column, group) hit table.
--only new|old runs one route alone, --runs times after one warm-up (for a kernel trace: launches per call = calls / (runs + 1)).

    python tools/bench_pipe_indices.py [--shapes scanner,and8] [--runs 5] [--old-runs 2] [--warmup 1] [--only new|old]
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
NBITS = 1_000_000_000


def build(ctx, shape, groups):
    rng = np.random.default_rng(3)
    pipe = bm.aggregator.pipeline(ctx, bm.agg_run_options(True, False))
    if shape == "scanner":
        planes = [bm.bvector.generate(ctx, SEED, 500 + i, 32768, NBITS) for i in range(32)]
        for _ in range(groups or 2048):
            x = int(rng.integers(1, 1 << 32))
            ag = pipe.add()
            for i in range(32):
                ag.add(planes[i], 0 if (x >> i) & 1 else 1)
        keep = planes
    else:
        av = [bm.bvector.generate(ctx, SEED, 100 + i, 655, NBITS, with_common=True) for i in range(48)]
        sv = [bm.bvector.generate(ctx, SEED, 200 + i, 655, NBITS) for i in range(16)]
        for _ in range(groups or 256):
            ag = pipe.add()
            for i in rng.choice(48, 8, replace=False): ag.add(av[int(i)], 0)
            for i in rng.choice(16, 2, replace=False): ag.add(sv[int(i)], 1)
        keep = av + sv
    pipe.complete()
    return pipe, keep


def route_new(agg, pipe):
    return agg.combine_and_sub_indices(pipe)


def route_old(agg, pipe):
    res = agg.combine_and_sub(pipe)
    parts = [r.to_indices() if r is not None else np.zeros(0, np.uint64) for r in res]
    offsets = np.zeros(len(parts) + 1, np.uint64)
    offsets[1:] = np.cumsum([p.size for p in parts], dtype=np.uint64)
    return offsets, (np.concatenate(parts) if parts else np.zeros(0, np.uint64))


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
    ap.add_argument("--shapes", default="scanner,and8")
    ap.add_argument("--groups", type=int, default=0, help="arg-groups per shape (0 = the shape's own number)")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--old-runs", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--only", choices=("new", "old"), default=None)
    args = ap.parse_args()
    ctx = bm.context(0)
    agg = bm.aggregator(ctx)
    for shape in args.shapes.split(","):
        pipe, keep = build(ctx, shape, args.groups)
        ncols = (NBITS + 65535) // 65536
        rec = {"shape": shape, "groups": pipe.size(), "columns": ncols, "operand_bytes": pipe.operand_bytes(),
               "table_bytes": pipe.size() * ncols * 12, "counts_plan": pipe.describe()}
        if args.only:
            fn = (lambda: route_new(agg, pipe)) if args.only == "new" else (lambda: route_old(agg, pipe))
            ts = [timed(fn, ctx)[0] for _ in range(args.runs + 1)][1:]
            rec[args.only] = stats(ts)
            print(json.dumps(rec), flush=True)
            del pipe, keep
            continue
        for _ in range(args.warmup):
            new = route_new(agg, pipe); old = route_old(agg, pipe)
        rec["identical"] = bool(new[0].shape == old[0].shape and (new[0] == old[0]).all() and new[1].shape == old[1].shape and (new[1] == old[1]).all())
        rec["hits"] = int(new[0][-1]); rec["groups_with_hits"] = int((np.diff(new[0].astype(np.int64)) > 0).sum())
        tn, to = [], []
        for k in range(max(args.runs, args.old_runs)):                    # alternating
            if k < args.runs: tn.append(timed(lambda: route_new(agg, pipe), ctx)[0])
            if k < args.old_runs: to.append(timed(lambda: route_old(agg, pipe), ctx)[0])
        rec["new"] = stats(tn); rec["old"] = stats(to)
        rec["speedup"] = round(rec["old"]["ms"] / rec["new"]["ms"], 2)
        print(json.dumps(rec), flush=True)
        del pipe, keep, new, old
        ctx.synchronize(); ctx.trim()
    ctx.close()


if __name__ == "__main__":
    main()
