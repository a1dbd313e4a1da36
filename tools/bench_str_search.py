#!/usr/bin/env python3
"""A batch of string lookups over one resident string column: the one-pass batch entry (bmx_slice_eq_keys, DESIGN_KERNELS.md 2.26)
against the counts pipeline with one AND-SUB group per string (the reference's find_eq_str(pipe), src/bmsparsevec_algo.h:3263),
over the same planes in the same process, alternating.  Both routes must give identical counts before anything is timed.

Column (from seeds): --rows 1e8 unique strings of 6..16 letters over a 20-letter alphabet, 16 octets = 128 planes.  The first six
letters spell the row number modulo 20^6 in base 20, the seventh tells the rows past 20^6 from those below: every row is unique by
construction.  Lengths are 6 + a geometric tail, so the planes of octets 13..15 are sparse and hold GAP blocks.
Cases, one JSON line each, for n in --n 1,16,256,4096,65536: n keys that are present (sampled rows), and n keys that are absent
(the seventh letter marks a row past 20^6 whose number is beyond --rows).  The pipeline holds a (block column, group) table of
operand pointers: it is run up to --pipe-max keys only (256: 0.4 GB at 1e8 rows; 4,096 groups would take 6 GB).

ms = host clock around the call (both routes end in a device synchronise), median of --runs after --warmup calls of each route, with
min / max = the run-to-run spread.  plane_bytes = what one pass of the batch kernel reads (bit-blocks of the planes + 8 KiB per block
column of every GAP-holding plane, which it reads expanded) x the passes the batch needs (keys per pass: what the LDS table holds).
probe = bmx_probe_stream_rw over plane_bytes of one pass on this box (2 reads : 1 write); entry_over_probe = ms per pass / probe ms.

    python tools/bench_str_search.py [--rows 100000000] [--n 1,16,256,4096,65536] [--pipe-max 256] [--runs 5] [--warmup 2]
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

ALPHABET = np.frombuffer(b"acdeghiklmnoprstuvwy", np.uint8)
OCTETS = 16
LOW = 20 ** 6
CHUNK = 1 << 24


def timed(fn, ctx):
    ctx.synchronize()
    t0 = time.perf_counter()
    out = fn()
    ctx.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def stats(ts):
    return {"ms": round(float(np.median(ts)), 3), "min": round(min(ts), 3), "max": round(max(ts), 3), "runs": len(ts)}


def spell(idx: np.ndarray, high: np.ndarray, seed: int) -> np.ndarray:
    """(n, 16) uint8: the strings of the row numbers idx (< 20^6) on the low / high side of 20^6"""
    rng = np.random.default_rng(seed)
    n = idx.size
    letters = rng.integers(0, 20, (n, OCTETS), dtype=np.uint8)
    x = idx.astype(np.int64)
    for j in range(6):
        letters[:, j] = x % 20
        x //= 20
    low7 = letters[:, 6]
    low7[low7 == 1] = 0                                                  # the seventh letter of a low row is never letter 1 ...
    letters[:, 6] = np.where(high, 1, low7)                              # ... which marks a high row
    length = 6 + np.minimum(rng.geometric(0.45, n) - 1, 10)
    length = np.where(high, np.maximum(length, 7), length)
    out = ALPHABET[letters]
    out[np.arange(OCTETS)[None, :] >= length[:, None]] = 0
    return out


def build_column(ctx, rows: int):
    """the planes on the device, built chunk by chunk: -> [bvector or None] * 128"""
    nwords = ((rows + 65535) // 65536) * 2048
    planes = [np.zeros(nwords, np.uint32) for _ in range(OCTETS * 8)]
    for lo in range(0, rows, CHUNK):
        hi = min(rows, lo + CHUNK)
        i = np.arange(lo, hi, dtype=np.int64)
        octets = spell(i % LOW, i >= LOW, 1000 + lo // CHUNK)
        for j in range(OCTETS):
            col = octets[:, j]
            for b in range(7):                                           # (letters are ASCII: bit 7 is never set)
                bits = np.packbits((col >> b) & 1, bitorder="little")
                planes[j * 8 + b].view(np.uint8)[lo // 8:lo // 8 + bits.size] = bits
    out = []
    for w in planes:
        out.append(bm.bit_import_u32(ctx, w, True) if w.any() else None)
    return out


def keys_for(rows: int, n: int, present: bool, rng) -> np.ndarray:
    if present:
        i = rng.choice(rows, size=n, replace=False).astype(np.int64) if n <= rows else None
        order = np.argsort(i)
        out = np.zeros((n, OCTETS), np.uint8)
        # a row's letters depend on its chunk's generator: spell whole chunks again, keep the sampled rows
        for c in np.unique(i // CHUNK):
            lo, hi = int(c) * CHUNK, min(rows, (int(c) + 1) * CHUNK)
            allr = np.arange(lo, hi, dtype=np.int64)
            octets = spell(allr % LOW, allr >= LOW, 1000 + int(c))
            sel = order[(i[order] // CHUNK) == c]
            out[sel] = octets[i[sel] - lo]
        return out
    x = rng.integers(max(rows - LOW, 0), LOW, n).astype(np.int64)       # the rows past 20^6 that do not exist
    return spell(x, np.ones(n, bool), 77)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=100_000_000)
    ap.add_argument("--n", default="1,16,256,4096,65536")
    ap.add_argument("--pipe-max", type=int, default=256)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    assert LOW < args.rows < 2 * LOW or args.rows <= LOW, "rows: up to 2 x 20^6"
    ctx = bm.context(0)
    t0 = time.perf_counter()
    planes = build_column(ctx, args.rows)
    sc = bm.str_scanner(ctx, planes, size=args.rows)
    ncols = (args.rows + 65535) // 65536
    info = [p.info()["counts"] for p in planes if p is not None]
    gap_planes = sum(1 for c in info if c[bm.GAP])
    pass_bytes = sum(c[bm.BIT] for c in info if not c[bm.GAP]) * 8192 + gap_planes * ncols * 8192
    keys_per_pass = 4394                                                 # 128 planes, 160 KiB of LDS (TUNING.md, eqk_pass_keys)
    pm = C.c_float()
    bm.check(bm.lib().bmx_probe_stream_rw(ctx._h, pass_bytes // 3 // 8192 * 8192, 3, 4, 12, C.byref(pm)))
    print(json.dumps({"column": {"rows": args.rows, "planes": len(info), "gap_holding_planes": gap_planes, "block_columns": ncols,
                                 "pass_bytes": pass_bytes, "build_s": round(time.perf_counter() - t0, 1),
                                 "probe_ms_for_pass_bytes": round(pm.value, 3)}}), flush=True)
    rng = np.random.default_rng(11)
    for n in (int(x) for x in args.n.split(",")):
        for present in (True, False):
            keys = keys_for(args.rows, n, present, rng)
            strs = [bytes(k).rstrip(b"\0") for k in keys]
            routes = {"entry": lambda: sc.eq_keys(keys, True, False)[0]}
            if n <= args.pipe_max:
                routes["pipeline"] = lambda: sc.find_eq_str_counts(strs, use_pipeline=True)
            out = {}
            for _ in range(args.warmup):
                for k, f in routes.items():
                    out[k] = f()
            rec = {"n": n, "keys": "present" if present else "absent", "sum_counts": int(out["entry"].sum()),
                   "identical": all(bool((out[k] == out["entry"]).all()) for k in routes)}
            assert rec["identical"] and rec["sum_counts"] == (n if present else 0), rec
            first = sc.eq_keys(keys, False, True)
            assert int(first[2].sum()) == (n if present else 0)
            ts = {k: [] for k in routes}
            for _ in range(args.runs):                                   # alternating
                for k, f in routes.items():
                    ts[k].append(timed(f, ctx)[0])
            for k in routes:
                rec[k] = stats(ts[k])
            passes = (n + keys_per_pass - 1) // keys_per_pass
            rec["passes"], rec["plane_bytes"] = passes, passes * pass_bytes
            rec["entry_ms_per_pass"] = round(rec["entry"]["ms"] / passes, 3)
            rec["entry_over_probe"] = round(rec["entry"]["ms"] / passes / pm.value, 2)
            rec["entry_GBps"] = round(passes * pass_bytes / rec["entry"]["ms"] / 1e6, 1)
            if "pipeline" in rec:
                rec["speedup"] = round(rec["pipeline"]["ms"] / rec["entry"]["ms"], 2)
                rec["entry_wins_beyond_spread"] = bool(rec["entry"]["max"] < rec["pipeline"]["min"])
            print(json.dumps(rec), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
