#!/usr/bin/env python3
"""A batch of range counts over one resident column (bmx_slice_range_counts, DESIGN_KERNELS.md 2.24) against the loop of
bmx_slice_compare(BMX_CMP_RANGE) count-only calls it replaces and leaves unchanged (tuning key rc_batch = -1).  Both routes run in
the same process, alternating, on the same column and the same ranges, and must give identical counts before anything is timed.

Column (from seeds): --planes 32 x --nbits 1e9 rows, every plane at 50 % -- the scanner workload of README.md.
Cases, one JSON line each, for n in --n 1,4,16,64,256:
  random      n ranges [a, a + w] with a, w uniform below 2^planes / 2^(planes - 3)
  histogram   n equal-width bins over [0, 2^planes): n + 1 edges, n closed ranges
and, with --batches 4,8, the batch route with rc_batch forced to each of them (thresholds per launch: which instantiation it takes).

ms = host clock around the call (both routes end in a device synchronise), median of --runs after --warmup calls of each route, with
min / max = the run-to-run spread.  launches / plane_bytes = what the batch route enqueued and the plane bytes its launches read
(counted by the kernel: bmx_slice_range_counts_stat), against all_planes_bytes = planes x rows / 8 per launch.
not_slower = the batch route's median is not above the loop's maximum (the acceptance rule: no slower than the loop beyond the
loop's own spread).

    python tools/bench_range_counts.py [--n 1,4,16,64,256] [--planes 32] [--nbits 1000000000] [--runs 7] [--warmup 2] [--batches 4,8]
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


def timed(fn, ctx):
    ctx.synchronize()
    t0 = time.perf_counter()
    out = fn()
    ctx.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def stats(ts):
    return {"ms": round(float(np.median(ts)), 3), "min": round(min(ts), 3), "max": round(max(ts), 3), "runs": len(ts)}


def cases(n: int, planes: int, rng):
    top = 1 << planes
    a = rng.integers(0, top, n, dtype=np.uint64)
    w = rng.integers(0, top >> 3, n, dtype=np.uint64)
    yield "random", [int(x) for x in a], [min(int(x) + int(y), top - 1) for x, y in zip(a, w)]
    edges = [top * k // n for k in range(n + 1)]
    yield "histogram", edges[:-1], [e - 1 for e in edges[1:]]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", default="1,4,16,64,256")
    ap.add_argument("--planes", type=int, default=32)
    ap.add_argument("--nbits", type=int, default=1_000_000_000)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--batches", default="")
    args = ap.parse_args()
    ctx = bm.context(0)
    sc = bm.slice_scanner(ctx, [bm.bvector.generate(ctx, SEED, 500 + i, 32768, args.nbits) for i in range(args.planes)], size=args.nbits)
    all_planes = args.planes * ((args.nbits + 65535) // 65536) * 8192
    rng = np.random.default_rng(11)
    forced = [int(b) for b in args.batches.split(",") if b]

    def route(batch):
        def run(lo, hi):
            ctx.set_tuning("rc_batch", batch)
            try:
                return sc.find_range_counts(lo, hi)
            finally:
                ctx.set_tuning("rc_batch", 0)
        return run

    for n in (int(x) for x in args.n.split(",")):
        for name, lo, hi in cases(n, args.planes, rng):
            rec = {"case": name, "n": n, "planes": args.planes, "rows": args.nbits, "all_planes_bytes": all_planes}
            routes = {"batch": route(0), "loop": route(-1)}
            for b in forced:
                routes["batch_%d" % b] = route(b)
            out = {}
            for _ in range(args.warmup):
                for k, f in routes.items():
                    out[k] = f(lo, hi)
            rec["identical"] = all(bool((out[k] == out["loop"]).all()) for k in routes)
            assert rec["identical"], rec
            rec["sum_counts"] = int(out["loop"].sum())
            ts = {k: [] for k in routes}
            for _ in range(args.runs):                                          # alternating
                for k, f in routes.items():
                    t, _ = timed(lambda: f(lo, hi), ctx)
                    ts[k].append(t)
            for k in routes:
                rec[k] = stats(ts[k])
            _, pb, launches = sc.range_counts_stat(lo, hi)
            rec["launches"], rec["plane_bytes"] = launches, pb
            rec["plane_bytes_per_launch_over_all_planes"] = round(pb / max(launches, 1) / all_planes, 3) if launches else None
            rec["speedup"] = round(rec["loop"]["ms"] / rec["batch"]["ms"], 2)
            rec["not_slower"] = bool(rec["batch"]["ms"] <= rec["loop"]["max"])
            print(json.dumps(rec), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
