"""bm::rank_compressor on the device (bmx_rank_compress / bmx_rank_decompress and the _many forms) against the route composed
of the entries the library had before, in the same run: bmx_vec_to_indices_dev -> bmx_rank_batch_dev / bmx_select_batch_dev ->
bmx_vec_from_indices_dev(BMX_SORTED), everything resident on the device.

One JSON line per case.  Times: device events around the call on the context's stream (bmx_timer_*), median of --runs runs
after --warmup runs.  Cases: idx = 1e9 bits at 50 %, 10 %, 1 % and 0.1 %; compress takes src = idx & (a 50 % vector), i.e. half
of idx; decompress takes the compress result, half of [0, count).  Every case runs under rankc_path -1 (automatic), 0
(positions) and 1 (blocks): the automatic choice has to be the faster one.  Reported per case: milliseconds, the algorithmic
bytes (bmx_vec_operand_bytes of idx and src plus those of the target), the fraction of 8 TB/s, the composed route's time and
whether both gave the same table.  With --batch: 32 sources in one _many call against 32 single calls.

    python tools/bench_rank_compress.py [--densities 32768,6554,655,66] [--runs 7] [--warmup 2] [--batch 32] [--nbits N]
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import bitmagic_amd as bm  # noqa: E402

SEED = 0xB17A61C
HBM_BS = 8e12


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


def _i64(n):
    t = torch.empty(max(n, 1), dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    return t


def route_compress(ctx, idx, rs, src, optimize):
    L = bm.lib()
    both = bm.bvector.bit_and(src, idx)
    cnt = both.count()
    ids, ranks = _i64(cnt), _i64(cnt)
    n = C.c_uint64()
    bm.check(L.bmx_vec_to_indices_dev(ctx._h, both._h, 8, C.c_void_p(ids.data_ptr()), cnt, C.byref(n)))
    if cnt:
        bm.check(L.bmx_rank_batch_dev(ctx._h, idx._h, rs._h, C.c_void_p(ids.data_ptr()), cnt, C.c_void_p(ranks.data_ptr())))
        ctx.synchronize()
        ranks -= 1
        torch.cuda.synchronize()
    return bm.bvector.from_indices(ctx, ranks[:cnt], rs.count(), bm.BM_SORTED, optimize)


def route_decompress(ctx, idx, rs, src, optimize):
    L = bm.lib()
    cnt = src.count()                                          # (src lies below count(idx) here)
    s, pos = _i64(cnt), _i64(cnt)
    found = torch.empty(max(cnt, 1), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    n = C.c_uint64()
    bm.check(L.bmx_vec_to_indices_dev(ctx._h, src._h, 8, C.c_void_p(s.data_ptr()), cnt, C.byref(n)))
    if cnt:
        ctx.synchronize()
        s += 1
        torch.cuda.synchronize()
        bm.check(L.bmx_select_batch_dev(ctx._h, idx._h, rs._h, C.c_void_p(s.data_ptr()), cnt, C.c_void_p(pos.data_ptr()),
                                        C.c_void_p(found.data_ptr())))
        ctx.synchronize()
    return bm.bvector.from_indices(ctx, pos[:cnt], idx.size(), bm.BM_SORTED, optimize)


def same_table(a, b):
    return a.size() == b.size() and all(x.shape == y.shape and (x == y).all() for x, y in zip(a.block_table(), b.block_table()))


def case(ctx, rc, name, direction, idx, rs, src, args):
    optimize = True
    call = (lambda: rc.compress_by_source(idx, rs, src, optimize)) if direction == "compress" else (lambda: rc.decompress(idx, src, rs, optimize))
    route = (lambda: route_compress(ctx, idx, rs, src, optimize)) if direction == "compress" else (lambda: route_decompress(ctx, idx, rs, src, optimize))
    rec = {"case": name, "direction": direction, "idx_bits": idx.size(), "idx_count": rs.count(), "src_count": src.count(), "optimize": 1}
    out = None
    for key, p in (("ms_positions", 0), ("ms_blocks", 1), ("ms", -1)):
        ctx.set_tuning("rankc_path", p)
        out = call()
        ms, ts = timed(ctx, call, args.runs, args.warmup)
        rec[key] = round(ms, 4)
        if p == -1:
            rec["ms_min"] = round(min(ts), 4)
    nb = idx.operand_bytes() + src.operand_bytes() + out.operand_bytes()
    rec["alg_bytes"] = nb
    rec["frac_8TBs"] = round(nb / HBM_BS * 1e3 / rec["ms"], 4)
    rec["auto_is_best"] = bool(rec["ms"] <= 1.05 * min(rec["ms_positions"], rec["ms_blocks"]))
    rv = route()
    rms, _ = timed(ctx, route, max(2, args.runs // 2), 1)
    rec["route_ms"] = round(rms, 4)
    rec["speedup_vs_route"] = round(rms / rec["ms"], 2)
    rec["route_equal"] = bool(same_table(out, rv))
    rec["out_counts"] = out.info()["counts"]
    print(json.dumps(rec), flush=True)
    return out


def batch(ctx, rc, name, direction, idx, rs, srcs, args):
    many = rc.compress_many if direction == "compress" else rc.decompress_many
    one = (lambda s: rc.compress_by_source(idx, rs, s, True)) if direction == "compress" else (lambda s: rc.decompress(idx, s, rs, True))
    ms_many, _ = timed(ctx, lambda: many(idx, srcs, rs, True), args.runs, args.warmup)
    ms_single, _ = timed(ctx, lambda: [one(s) for s in srcs], args.runs, args.warmup)
    outs = many(idx, srcs, rs, True)
    eq = all(same_table(o, one(s)) for o, s in zip(outs[:4], srcs[:4]))
    print(json.dumps({"case": name, "direction": direction + "_many", "sources": len(srcs), "ms_many": round(ms_many, 4),
                      "ms_singles": round(ms_single, 4), "many_vs_singles": round(ms_single / ms_many, 2), "equal": bool(eq)}), flush=True)
    return outs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--densities", default="32768,6554,655,66")
    ap.add_argument("--nbits", type=int, default=1_000_000_000)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--batch", type=int, default=32)
    args = ap.parse_args()
    ctx = bm.context(0)
    rc = bm.rank_compressor(ctx)
    for dq in [int(x) for x in args.densities.split(",")]:
        name = "idx %.4g%%" % (dq / 655.36)
        idx = bm.bvector.generate(ctx, SEED, 0, dq, args.nbits, optimize=True)
        rs = idx.build_rs_index()
        src = bm.bvector.bit_and(idx, bm.bvector.generate(ctx, SEED, 1, 32768, args.nbits, optimize=True), bm.opt_compress)
        comp = case(ctx, rc, name, "compress", idx, rs, src, args)
        case(ctx, rc, name, "decompress", idx, rs, comp, args)
        if args.batch:
            ctx.set_tuning("rankc_path", -1)
            srcs = [bm.bvector.bit_and(idx, bm.bvector.generate(ctx, SEED, 2 + i, 32768, args.nbits, optimize=True), bm.opt_compress)
                    for i in range(args.batch)]
            outs = batch(ctx, rc, name, "compress", idx, rs, srcs, args)
            del srcs
            batch(ctx, rc, name, "decompress", idx, rs, outs, args)
            del outs
        del comp, src, rs, idx
        ctx.synchronize(); ctx.trim()
    ctx.close()


if __name__ == "__main__":
    main()
