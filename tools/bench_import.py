"""Vectors from lists of bit positions on the device (bvector::set(ids, n, sort_order) on an empty vector; bmx_vec_from_indices_dev)
against today's route in the same run: the ids to the host, a NumPy scatter into raw words, bm.bit_import_u32.

One JSON line per workload.  Times: device events around the call on the context's stream, median of --runs runs after --warmup
runs (the route: host clock around the whole route, median of --route-runs).  Bounds at 8 TB/s (DESIGN_KERNELS.md 2.19):
  one_pass  the ids read once + the vector written once (descriptor table, bit slab, GAP slab)
  path      what the path itself moves: the ids once per pass that reads them (sorted: bounds, starts, [stats,] emit;
            any other order: bounds, histogram, scatter), the 16-bit buckets written once and read by [stats and] emit
Workloads (data set A = bm.bvector.generate(seed, v, density_q16, 1e9 bits)):
  1  1e9 bits at 10 %: 1e8 sorted u32 ids from bmx_vec_to_indices_dev, optimize 0 and 1
  2  the same ids shuffled on the device (the unsorted path), optimize 0 and 1
  3  1e9 bits at 1 %, optimize 1 (GAP and bit-blocks)
  4  1e5 random ids over 2^32 bits (width 4) and over 2^36 bits (width 8), optimize 1
  5  (with every workload above that fits in host words: 1-3 and 4 at 2^32 bits) today's route

    python tools/bench_import.py [--workloads 1,2,3,4] [--runs 20] [--warmup 3] [--route-runs 3]
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import bitmagic_amd as bm  # noqa: E402

SEED = 0xB17A61C
HBM_BS = 8e12
NBITS = 1_000_000_000


def timed(ctx, fn, runs, warmup):
    for _ in range(warmup):
        fn()
    ctx.synchronize()
    ts = []
    for _ in range(runs):
        ctx.timer_start()
        fn()
        ts.append(ctx.timer_stop_ms())
    return float(np.median(ts)), ts


def device_ids(ctx, v, width):
    """the vector's set bits as a device tensor (bmx_vec_to_indices_dev): no host copy"""
    cnt = v.count()
    d = torch.empty(cnt, dtype=torch.int32 if width == 4 else torch.int64, device="cuda")
    torch.cuda.synchronize()
    n = C.c_uint64()
    bm.check(bm.lib().bmx_vec_to_indices_dev(ctx._h, v._h, width, C.c_void_p(d.data_ptr()), cnt, C.byref(n)))
    ctx.synchronize()
    return d


def out_bytes(v):
    i = v.info()
    return i["nblocks"] * 8 + i["counts"][bm.BIT] * 8192 + i["gap_words"] * 2


def route(ctx, d, nbits, optimize):
    """today's route: ids to the host, scatter into raw 32-bit words, bit_import_u32 -> (vector, ms)"""
    t0 = time.perf_counter()
    ids = d.cpu().numpy().view(np.uint32 if d.element_size() == 4 else np.uint64).astype(np.uint64)
    words = np.zeros((nbits + 31) // 32, np.uint32)
    np.bitwise_or.at(words, ids >> np.uint64(5), (np.uint32(1) << (ids & np.uint64(31)).astype(np.uint32)))
    v = bm.bit_import_u32(ctx, words, optimize)
    ctx.synchronize()
    return v, (time.perf_counter() - t0) * 1e3


def workload(ctx, name, d, nbits, so, optimize, sorted_path, args, with_route):
    n, width = d.numel(), d.element_size()
    v = bm.bvector.from_indices(ctx, d, nbits, so, optimize)
    ms, ts = timed(ctx, lambda: bm.bvector.from_indices(ctx, d, nbits, so, optimize), args.runs, args.warmup)
    ob, ib = out_bytes(v), n * width
    passes = (3 + (1 if optimize else 0)) if sorted_path else 3
    path_b = ib * passes + ob + (0 if sorted_path else n * 2 * (2 + (1 if optimize else 0)))
    rec = {"workload": name, "n_ids": n, "width": width, "nbits": nbits, "sort_order": so, "optimize": int(optimize),
           "path": "sorted" if sorted_path else "bucketed", "ms": round(ms, 4), "ms_min": round(min(ts), 4),
           "ids_per_s": n / (ms * 1e-3), "counts": v.info()["counts"], "out_bytes": ob, "ids_bytes": ib,
           "one_pass_bound_ms": round((ib + ob) / HBM_BS * 1e3, 4), "path_bound_ms": round(path_b / HBM_BS * 1e3, 4)}
    rec["frac_one_pass_bound"] = round(rec["one_pass_bound_ms"] / ms, 3)
    rec["frac_path_bound"] = round(rec["path_bound_ms"] / ms, 3)
    if with_route and args.route_runs:
        rms = []
        for _ in range(args.route_runs):
            rv, t = route(ctx, d, v.size(), optimize)
            rms.append(t)
        rec["route_ms"] = round(float(np.median(rms)), 2)
        rec["speedup_vs_route"] = round(rec["route_ms"] / ms, 1)
        nw = v.info()["nblocks"] * bm.BLOCK_WORDS
        rec["route_equal"] = bool((rv.to_words(nw) == v.to_words(nw)).all()) and rv.count() == v.count()
        del rv
    print(json.dumps(rec), flush=True)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="1,2,3,4")
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--route-runs", type=int, default=3)
    args = ap.parse_args()
    wl = {int(x) for x in args.workloads.split(",")}
    ctx = bm.context(0)
    if wl & {1, 2}:
        a = bm.bvector.generate(ctx, SEED, 0, 6554, NBITS, optimize=True)
        d = device_ids(ctx, a, 4)
        del a
        if 1 in wl:
            for opt in (False, True):
                workload(ctx, "W1 10% sorted", d, NBITS, bm.BM_SORTED, opt, True, args, True)
        if 2 in wl:
            g = torch.Generator(device="cuda").manual_seed(SEED)
            ds = d[torch.randperm(d.numel(), device="cuda", generator=g)].contiguous()
            torch.cuda.synchronize()
            for opt in (False, True):
                workload(ctx, "W2 10% shuffled", ds, NBITS, bm.BM_UNKNOWN, opt, False, args, True)
            del ds
        del d
    if 3 in wl:
        a = bm.bvector.generate(ctx, SEED, 1, 655, NBITS, optimize=True)
        d = device_ids(ctx, a, 4)
        del a
        workload(ctx, "W3 1% sorted", d, NBITS, bm.BM_SORTED, True, True, args, True)
        del d
    if 4 in wl:
        rng = np.random.default_rng(SEED)
        for bits, width in ((32, 4), (36, 8)):
            ids = rng.integers(0, 1 << bits, size=100_000, dtype=np.uint64)
            ids[0] = (1 << bits) - 1
            host = ids.astype(np.uint32).view(np.int32) if width == 4 else ids.view(np.int64)
            d = torch.from_numpy(host.copy()).cuda()
            torch.cuda.synchronize()
            workload(ctx, f"W4 1e5 random ids over 2^{bits} bits", d, 0, bm.BM_UNKNOWN, True, False, args, bits == 32)
    ctx.close()


if __name__ == "__main__":
    main()
