"""Device intervals (bmx_vec_from_ranges_dev, bmx_vec_to_ranges_dev; DESIGN_KERNELS.md 2.20) against the route through bit
positions in the same process, alternating with the new call:
  from:  positions expanded on the device (torch.repeat_interleave / arange) into bmx_vec_from_indices_dev(..., optimize=1)
  to:    bmx_vec_to_indices_dev plus a torch diff / compaction

One JSON line per workload and repeat.  ms: device events around the new call on the context's stream, median of --runs after
--warmup; ms_wall / route_ms: host clock around the whole call / route (the route spans two streams), median of the same runs.
bound_bytes: what the path must move -- pairs read + table written (R), table read + pairs written (T) -- and its fraction of
the 8 TB/s HBM peak.  Every line is repeated --repeats times; spread = (max - min) / median of the repeats' ms.
Workloads, 1e9-bit vectors, 64-bit pairs as a device tensor, all from seeds:
  R1  2e6 sorted separated pairs, mean length 100 (every block GAP, ~260 runs)
  R2  5e7 sorted separated pairs, mean length 5 (every block a bit-block)
  R3  the pairs of R1 shuffled, 10 % of them duplicated and stretched to overlap
  R4  1,000 pairs of ~5e5 bits (mostly FULL blocks)
  T1-T4  to_ranges_dev of the four vectors

    python tools/bench_ranges.py [--workloads R1,R2,R3,R4,T1,T2,T3,T4] [--runs 20] [--warmup 3] [--repeats 3]
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


def pairs_of(name: str) -> np.ndarray:
    rng = np.random.default_rng(SEED)
    if name in ("R1", "R3"):
        i = np.arange(2_000_000, dtype=np.int64)
        l = i * 500 + rng.integers(0, 200, i.size)
        p = np.stack([l, l + rng.integers(0, 199, i.size)], axis=1)          # (ends <= slot + 397: separated)
        if name == "R3":
            extra = p[rng.choice(p.shape[0], p.shape[0] // 10, replace=False)].copy()
            extra[:, 1] += rng.integers(0, 600, extra.shape[0])
            p = np.concatenate([p, extra])
            rng.shuffle(p, axis=0)
        return p
    if name == "R2":
        i = np.arange(50_000_000, dtype=np.int64)
        l = i * 20 + rng.integers(0, 6, i.size)
        return np.stack([l, l + rng.integers(0, 9, i.size)], axis=1)
    i = np.arange(1000, dtype=np.int64)
    l = i * 1_000_000 + rng.integers(0, 100_000, i.size)
    return np.stack([l, l + rng.integers(400_000, 600_000, i.size)], axis=1)


def expand(d: torch.Tensor) -> torch.Tensor:
    """every position the pairs cover, in pair order (duplicates where pairs overlap)"""
    lens = d[:, 1] - d[:, 0] + 1
    first = torch.cumsum(lens, 0) - lens
    return torch.repeat_interleave(d[:, 0] - first, lens) + torch.arange(int(lens.sum()), device=d.device, dtype=d.dtype)


def route_from(ctx, d, nbits):
    ids = expand(d).contiguous()
    torch.cuda.synchronize()
    return bm.bvector.from_indices(ctx, ids, nbits, bm.BM_UNKNOWN, True)


def to_ranges_dev(ctx, v, out):
    n = v.to_ranges_dev(out)
    ctx.synchronize()
    return out[:n]


def route_to(ctx, v, ids_buf):
    n = C.c_uint64()
    bm.check(bm.lib().bmx_vec_to_indices_dev(ctx._h, v._h, 8, C.c_void_p(ids_buf.data_ptr()), ids_buf.numel(), C.byref(n)))
    ctx.synchronize()
    idx = ids_buf[:n.value]
    brk = idx[1:] != idx[:-1] + 1
    one = torch.ones(1, dtype=torch.bool, device=idx.device)
    out = torch.stack([idx[torch.cat([one, brk])], idx[torch.cat([brk, one])]], dim=1)
    torch.cuda.synchronize()
    return out


def measure(ctx, new, old, runs, warmup):
    for _ in range(warmup):
        new(); old()
    ctx.synchronize(); torch.cuda.synchronize()
    ev, wall, rt = [], [], []
    for _ in range(runs):
        t0 = time.perf_counter()
        ctx.timer_start(); new(); ev.append(ctx.timer_stop_ms())
        ctx.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter()
        old()
        ctx.synchronize(); torch.cuda.synchronize()
        rt.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ev)), float(np.median(wall)), float(np.median(rt))


def table_bytes(v):
    i = v.info()
    return i["nblocks"] * 8 + i["counts"][bm.BIT] * 8192 + i["gap_words"] * 2


def report(rec, reps):
    ms = [r[0] for r in reps]
    med = float(np.median(ms))
    rec.update({"ms": round(med, 4), "ms_repeats": [round(x, 4) for x in ms], "spread": round((max(ms) - min(ms)) / med, 3),
                "ms_wall": round(float(np.median([r[1] for r in reps])), 4), "route_ms": round(float(np.median([r[2] for r in reps])), 4)})
    rec["bound_ms"] = round(rec["bound_bytes"] / HBM_BS * 1e3, 5)
    rec["frac_hbm_bound"] = round(rec["bound_ms"] / med, 4)
    rec["speedup_vs_route_wall"] = round(rec["route_ms"] / rec["ms_wall"], 2)
    print(json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="R1,R2,R3,R4,T1,T2,T3,T4")
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args()
    wl = set(args.workloads.split(","))
    ctx = bm.context(0)
    for k in ("1", "2", "3", "4"):
        if not ({"R" + k, "T" + k} & wl):
            continue
        p = pairs_of("R" + k)
        d = torch.from_numpy(p).cuda().contiguous()
        torch.cuda.synchronize()
        v = bm.bvector.from_ranges(ctx, d, NBITS)
        info = v.info()
        covered = v.count()
        if "R" + k in wl:
            rv = route_from(ctx, d, NBITS)
            same = bm.count_xor(v, rv) == 0 and rv.count() == covered and rv.info()["counts"] == info["counts"]
            del rv
            rec = {"workload": "R" + k, "pairs": int(p.shape[0]), "covered_bits": covered, "counts": info["counts"],
                   "pairs_bytes": int(p.nbytes), "table_bytes": table_bytes(v), "route_ids_bytes": int((p[:, 1] - p[:, 0] + 1).sum()) * 8,
                   "bound_bytes": int(p.nbytes) + table_bytes(v), "route_count_xor_0": bool(same)}
            reps = [measure(ctx, lambda: bm.bvector.from_ranges(ctx, d, NBITS), lambda: route_from(ctx, d, NBITS), args.runs, args.warmup)
                    for _ in range(args.repeats)]
            report(rec, reps)
        if "T" + k in wl:
            n = C.c_uint64()
            bm.lib().bmx_vec_to_ranges_dev(ctx._h, v._h, 8, None, 0, C.byref(n))
            out = torch.empty((max(n.value, 1), 2), dtype=torch.int64, device="cuda")
            ids_buf = torch.empty(covered, dtype=torch.int64, device="cuda")
            torch.cuda.synchronize()
            got = to_ranges_dev(ctx, v, out)
            same = bool(torch.equal(got, route_to(ctx, v, ids_buf)))
            rec = {"workload": "T" + k, "intervals": int(n.value), "covered_bits": covered, "counts": info["counts"],
                   "table_bytes": table_bytes(v), "out_bytes": int(n.value) * 16, "route_ids_bytes": covered * 8,
                   "bound_bytes": table_bytes(v) + int(n.value) * 16, "route_equal_intervals": same}
            reps = [measure(ctx, lambda: to_ranges_dev(ctx, v, out), lambda: route_to(ctx, v, ids_buf), args.runs, args.warmup)
                    for _ in range(args.repeats)]
            report(rec, reps)
            del out, ids_buf
        del v, d
    ctx.close()


if __name__ == "__main__":
    main()
