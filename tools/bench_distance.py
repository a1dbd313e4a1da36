"""All-pairs distance matrices and bm::distance_operation on the device (bmx_distance_matrix_dev, bmx_distance) against
today's route in the same run: one 2-operand AND group per pair in a counts-only pipeline, and bm::count_* calls.

One JSON line per workload.  Times: device events around the call on the context's stream, median of --runs runs after
--warmup runs (the route: median of --route-runs).  Derived bounds (DESIGN_KERNELS.md 2.18):
  VALU ceiling  256 CUs x 64 lanes x 2.4 GHz = 39.3e12 32-bit lane-ops/s; one v_and_b32 + one v_bcnt_u32_b32 per 32
                bit-pairs -> 6.29e14 bit-pairs/s
  HBM bound     the operand bytes the tiling must read (every vector once per tile it belongs to) at 8 TB/s

    python tools/bench_distance.py [--workloads 1,2,3,4,5] [--runs 20] [--route-runs 3]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import bitmagic_amd as bm  # noqa: E402

SEED = 0xB17A61C
VALU_BITPAIRS_S = 256 * 64 * 2.4e9 * 32 / 2
HBM_BS = 8e12
TILE = 64


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


def tiled_bytes(A, B):
    """operand bytes the tile kernel reads: a vector once per tile pair it belongs to"""
    ob = lambda v: v.operand_bytes() if v is not None else 0
    if B is None:
        t = (len(A) + TILE - 1) // TILE
        return sum(ob(v) for v in A) * t
    ta, tb = (len(A) + TILE - 1) // TILE, (len(B) + TILE - 1) // TILE
    return sum(ob(v) for v in A) * tb + sum(ob(v) for v in B) * ta


def matrix_workload(ctx, name, A, B, nbits, args):
    sym = B is None
    nb = len(A) if sym else len(B)
    d_and = torch.zeros(len(A) * nb, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    ms, ts = timed(ctx, lambda: bm.distance_matrix_dev(A, B, d_and.data_ptr(), ctx=ctx), args.runs, args.warmup)
    ctx.synchronize()
    got = d_and.cpu().numpy().astype(np.uint64).reshape(len(A), nb)
    pairs = len(A) * (len(A) + 1) // 2 if sym else len(A) * nb          # distinct pairs (symmetric: with the diagonal)
    bitpairs = pairs * nbits
    rate = bitpairs / (ms * 1e-3)
    rd = tiled_bytes(A, B)
    out = {"workload": name, "na": len(A), "nb": nb, "symmetric": sym, "nbits": nbits, "ms": round(ms, 4),
           "ms_min": round(min(ts), 4), "ms_max": round(max(ts), 4), "pairs": pairs, "bit_pairs_per_s": float("%.4g" % rate),
           "frac_valu_ceiling": round(rate / VALU_BITPAIRS_S, 4), "tiled_read_bytes": rd,
           "frac_hbm_bound": round((rd / HBM_BS) / (ms * 1e-3), 4)}
    out["binds"] = "valu" if bitpairs / VALU_BITPAIRS_S >= rd / HBM_BS else "hbm"
    if args.route_runs > 0:
        idx = [(i, j) for i in range(len(A)) for j in (range(i, nb) if sym else range(nb))]
        pipe = bm.aggregator.pipeline(ctx)
        for i, j in idx:
            g = pipe.add()
            g.add(A[i], 0)
            g.add(A[j] if sym else B[j], 0)
        pipe.complete()
        agg = bm.aggregator(ctx)
        d_cnt = torch.zeros(len(idx), dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        rms, _ = timed(ctx, lambda: agg.run_counts_dev(pipe, d_cnt.data_ptr()), args.route_runs, 1)
        ctx.synchronize()
        cnt = d_cnt.cpu().numpy().astype(np.uint64)
        ii = np.array([p[0] for p in idx]); jj = np.array([p[1] for p in idx])
        out["route_pipeline_ms"] = round(rms, 3)
        out["speedup_vs_route"] = round(rms / ms, 2)
        out["equal_to_route"] = bool((got[ii, jj] == cnt).all() and (not sym or (got[jj, ii] == cnt).all()))
        del pipe
    print(json.dumps(out), flush=True)
    return out


def pair_workload(ctx, args):
    nbits = 1_000_000_000
    a = bm.bvector.generate(ctx, SEED, 1, 6554, nbits, with_common=True)
    b = bm.bvector.generate(ctx, SEED, 2, 6554, nbits, with_common=True)
    m3 = (bm.COUNT_AND, bm.COUNT_A, bm.COUNT_B)
    ms_d, _ = timed(ctx, lambda: bm.distance_operation(a, b, m3), args.runs, args.warmup)
    ms_and, _ = timed(ctx, lambda: bm.count_and(a, b), args.runs, args.warmup)
    # today's three calls and three passes: count_and, count, count
    ms_3, _ = timed(ctx, lambda: (bm.count_and(a, b), a.count(), b.count()), args.runs, args.warmup)
    got = bm.distance_operation(a, b, m3)
    exp = [bm.count_and(a, b), a.count(), b.count()]
    out = {"workload": "4_pair_and_a_b", "nbits": nbits, "ms": round(ms_d, 4), "count_and_ms": round(ms_and, 4),
           "three_calls_ms": round(ms_3, 4), "ratio_vs_count_and": round(ms_d / ms_and, 3),
           "ratio_vs_three_calls": round(ms_d / ms_3, 3), "bytes": a.operand_bytes() + b.operand_bytes(),
           "frac_hbm_bound": round(((a.operand_bytes() + b.operand_bytes()) / HBM_BS) / (ms_d * 1e-3), 4),
           "equal": got == exp}
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="1,2,3,4,5")
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--route-runs", type=int, default=3)
    ap.add_argument("--scale", type=float, default=1.0, help="multiply every vector length (rehearsals)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_distance: no GPU")
    s = torch.cuda.Stream()
    torch.cuda.set_stream(s)
    ctx = bm.context(0, s.cuda_stream)
    wl = {int(x) for x in args.workloads.split(",") if x}
    sc = lambda n: max(65536, int(n * args.scale))
    if 1 in wl:
        nbits = sc(1_000_000_000)
        A = [bm.bvector.generate(ctx, SEED, i, 6554, nbits, with_common=True) for i in range(256)]
        matrix_workload(ctx, "1_sym_256_dataset_A", A, None, nbits, args)
        del A
        ctx.trim()
    if 2 in wl:
        nbits = sc(1_000_000_000)
        A = [bm.bvector.generate(ctx, SEED, 300 + i, 32768, nbits) for i in range(32)]
        matrix_workload(ctx, "2_scanner_32_planes_50pct", A, None, nbits, args)
        del A
        ctx.trim()
    if 3 in wl:
        nbits = sc(100_000_000)
        A = [bm.bvector.generate(ctx, SEED, 400 + i, 655, nbits) for i in range(64)]
        B = [bm.bvector.generate(ctx, SEED, 500 + i, 655, nbits) for i in range(1024)]
        matrix_workload(ctx, "3_asym_64x1024_mixed_1pct", A, B, nbits, args)
        del A, B
        ctx.trim()
    if 4 in wl:
        pair_workload(ctx, args)
        ctx.trim()
    if 5 in wl:
        nbits = sc(100_000_000)
        A = [bm.bvector.generate(ctx, SEED, 600 + i, 197, nbits) for i in range(64)]
        matrix_workload(ctx, "5_sym_64_all_gap_0.3pct", A, None, nbits, args)
        del A
    ctx.synchronize()


if __name__ == "__main__":
    main()
