#!/usr/bin/env python3
"""The values of the selected rows of a resident column (bmx_slice_values_dev) and the image of the selection under it
(bmx_slice_remap: set2set_11_transform::remap), DESIGN_KERNELS.md 2.25, next to the two ends of the call WITHOUT the decode:
bmx_vec_to_indices_dev of the selection + bmx_vec_from_indices_dev of that list (existing code, timed in the same process on the
same selection: the floor comes from code that is not under test).

Column (from seeds): 32 planes x 1e9 rows.  Planes 0..29 are random at 50 %, so the values are uniform below 2^30 = 1.07e9; planes 30
and 31 hold no bit, as they would for values below 1e9 (their blocks are NULL: skipped without a read).  No not-NULL vector unless
--not-null (95 %).  Selections: 1e3 and 1e6 uniformly random rows, 1e8 rows (every row with probability 0.1), and 1e6 clustered
rows (1,000 runs of 1,000 consecutive rows).

One JSON line per selection:
  values_dev / remap / floor   ms = host clock around the call (each ends in a device synchronise), median of --runs after --warmup,
                               with min / max = the run-to-run spread; floor = to_indices_dev + from_indices_dev, with its two parts
  algorithmic_bytes            descriptor-counted blocks of the TOUCHED columns (those with a selected row): 8,192 B per bit-block,
                               2 x (len + 1) B per GAP block of the planes, the not-NULL vector and the selector, plus the list written
  hbm_fraction                 those bytes over the values_dev time over the 8.0 TB/s peak
  remap_over_floor             remap ms / floor ms
  us_per_touched_column        values_dev time over the touched columns (the figure a path for columns with very few selected rows
                               would be judged by: at 1e6 random rows a touched column holds about 65 of them)

    python tools/bench_remap.py [--rows 1000000000] [--selections 1e3,1e6,1e8,clustered] [--runs 7] [--warmup 2] [--not-null]
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

import bitmagic_amd as bm  # noqa: E402

SEED = 0xB17A61C
HBM_PEAK = 8.0e12
B = 65536


def selection(ctx, name: str, rows: int):
    """-> (bvector, touched block columns)"""
    rng = np.random.default_rng(2025)
    if name == "1e8":
        # every row with probability 0.1: every column is touched
        return bm.bvector.generate(ctx, SEED, 950, 6554, rows), (rows + B - 1) // B
    if name == "clustered":
        starts = np.sort(rng.integers(0, rows - 1000, 1000, dtype=np.uint64))
        v = bm.bvector.from_ranges(ctx, np.stack([starts, starts + np.uint64(999)], axis=1), rows)
        ids = (starts[:, None] + np.arange(1000, dtype=np.uint64)[None, :]).reshape(-1)
    else:
        ids = rng.integers(0, rows, int(float(name)), dtype=np.uint64)
        v = bm.bvector.from_indices(ctx, ids, rows, bm.BM_UNSORTED, True)
    return v, int(np.unique(ids >> np.uint64(16)).size)


def touched_bytes(v, touched: int) -> int:
    """descriptor-counted bytes of v's blocks in the touched columns: exact for a vector whose blocks are all of one size (the
    planes: all bit-blocks or all NULL), proportional otherwise"""
    nb = v.info()["nblocks"]
    return int(round(v.operand_bytes() * touched / nb)) if nb else 0


def timed(fn, ctx):
    ctx.synchronize()
    t0 = time.perf_counter()
    out = fn()
    ctx.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def stats(ts):
    return {"ms": round(float(np.median(ts)), 3), "min": round(min(ts), 3), "max": round(max(ts), 3), "runs": len(ts)}


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000_000)
    ap.add_argument("--selections", default="1e3,1e6,1e8,clustered")
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--not-null", action="store_true")
    args = ap.parse_args()
    ctx = bm.context(0)
    L = bm.lib()
    rows = args.rows
    planes = [bm.bvector.generate(ctx, SEED, 700 + i, 32768, rows) for i in range(30)]
    planes += [bm.bvector.from_indices(ctx, np.zeros(0, np.uint32), rows) for _ in range(2)]
    nn = bm.bvector.generate(ctx, SEED, 940, 62259, rows) if args.not_null else None
    col = bm.slice_scanner(ctx, planes, size=rows, not_null=nn)
    t = bm.set2set_11_transform(ctx)
    for name in args.selections.split(","):
        sel, touched = selection(ctx, name, rows)
        n = sel.count() if nn is None else bm.count_and(sel, nn)
        n_sel = sel.count()
        d_val = torch.empty(max(n_sel, 1), dtype=torch.int32, device="cuda")
        d_ids = torch.empty(max(n_sel, 1), dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        rec = {"selection": name, "rows": rows, "planes": len(planes), "not_null": nn is not None, "selected_rows": int(n),
               "touched_columns": touched, "columns": (rows + B - 1) // B}
        rec["algorithmic_bytes"] = (sum(touched_bytes(p, touched) for p in planes) + (touched_bytes(nn, touched) if nn is not None else 0)
                                    + sel.operand_bytes() + 4 * int(n))

        def values_dev():
            return col.values_dev(d_val.data_ptr(), n_sel, sel, None, 4)

        def remap():
            return t.remap(sel, col)

        cnt = C.c_uint64()
        part = {}

        def floor():
            h = C.c_void_p()
            t0 = time.perf_counter()
            bm.check(L.bmx_vec_to_indices_dev(ctx._h, sel._h, 4, C.c_void_p(d_ids.data_ptr()), n_sel, C.byref(cnt)))
            ctx.synchronize()
            t1 = time.perf_counter()
            bm.check(L.bmx_vec_from_indices_dev(ctx._h, C.c_void_p(d_ids.data_ptr()), 4, cnt.value, bm.BM_UNSORTED, rows, 1, C.byref(h)))
            ctx.synchronize()
            part.setdefault("to_indices_dev", []).append((t1 - t0) * 1e3)
            part.setdefault("from_indices_dev", []).append((time.perf_counter() - t1) * 1e3)
            return bm.bvector(ctx, h)

        for _ in range(args.warmup):
            assert values_dev() == n
            img = remap(); back = floor()
        rec["image_count"] = img.count()
        rec["floor_round_trip_identical"] = bool(bm.count_xor(back, sel) == 0)
        # the device list against the image: the vector of the list IS the image
        again = bm.bvector.from_indices(ctx, d_val[:n], 0, bm.BM_UNSORTED, True)
        rec["image_is_the_vector_of_the_list"] = bool(again.size() == img.size() and bm.count_xor(again, img) == 0)
        del img, back, again
        part.clear()
        tv, tr, tf = [], [], []
        for _ in range(args.runs):                                          # alternating
            ms, _ = timed(values_dev, ctx); tv.append(ms)
            ms, r = timed(remap, ctx); tr.append(ms); del r
            ms, r = timed(floor, ctx); tf.append(ms); del r
        rec["values_dev"], rec["remap"], rec["floor"] = stats(tv), stats(tr), stats(tf)
        rec["floor_parts"] = {k: round(float(np.median(v)), 3) for k, v in part.items()}
        rec["remap_over_floor"] = round(rec["remap"]["ms"] / rec["floor"]["ms"], 2)
        rec["hbm_fraction"] = round(rec["algorithmic_bytes"] / (rec["values_dev"]["ms"] * 1e-3) / HBM_PEAK, 4)
        rec["us_per_touched_column"] = round(rec["values_dev"]["ms"] * 1e3 / max(touched, 1), 3)
        print(json.dumps(rec), flush=True)
        del sel, d_val, d_ids
    ctx.close()


if __name__ == "__main__":
    main()
