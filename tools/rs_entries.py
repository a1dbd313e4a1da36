#!/usr/bin/env python3
"""Every path of the rank / select family (bmx_rs_build and its stages, rank_plan / rank_launch, select_plan / select_launch, the
host round trip, running_counts in bmx.hip), once, at small sizes: what a launch / synchronise / copy / allocation count is taken
over (profiles/refactor_rs).  Run it under `rocprofv3 --kernel-trace --hip-trace --stats -- python tools/rs_entries.py` against two
builds (BMX_LIB) and compare the tables; it prints one JSON line per case with info() of the index and a sha256 of the rank answers,
the select positions and the found flags, so that two builds can be held against each other line for line.

Vectors: the empty one; 23 blocks of every kind (NULL, FULL, bit, three shapes of GAP); 40 dense blocks that keep 16-bit select
lines; 2,000 GAP blocks of three ones each (bmx_rs_build drops the directory's summary).  Index builds: rs_lines 0 / 1 / 2,
rs_select_sel -1 / 0 / 1 / 2, rs_sdir_shift 0 / 6 / 16.  Queries: rs_lanes 0 / 2 / 4 / 8, rs_select_lines 0 / 1 / 2, rs_select_top
-1 / 0 / 1, rs_sorted_hint 0 / 1 (ascending batches), rs_select_sel 0 over an index that holds select lines; batches of 1, 65,535
and 65,536 (the automatic lanes), 2^22 (k_select_top) where the index has a summary.  Then to_indices and rank_compress /
rank_decompress with and without an index: the two callers of running_counts."""
import hashlib, itertools, json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import bitmagic_amd as bm

SEED = 0xB17A61C
BUILD_KEYS = {"rs_lines": 1, "rs_select_sel": -1, "rs_sdir_shift": 0}
QUERY_KEYS = {"rs_lanes": 0, "rs_select_lines": 2, "rs_select_top": -1, "rs_sorted_hint": 0}
BUILDS = ({"rs_lines": 0, "rs_select_sel": 0}, {}, {"rs_lines": 2, "rs_select_sel": 0}, {"rs_lines": 2, "rs_select_sel": 0, "rs_sdir_shift": 6},
          {"rs_lines": 2, "rs_select_sel": 0, "rs_sdir_shift": 16}, {"rs_lines": 2, "rs_select_sel": 1}, {"rs_lines": 0, "rs_select_sel": 2})
ctx = bm.context(0)


def sha(x):
    return hashlib.sha256(np.ascontiguousarray(x).tobytes()).hexdigest()[:16]


def tune(defaults, knobs):
    for k, x in {**defaults, **knobs}.items(): ctx.set_tuning(k, x)
    return ",".join(f"{k}={x}" for k, x in knobs.items()) or "default"


def mixed_words(nblk=23):
    rng = np.random.default_rng(23)
    w = np.zeros(nblk * 2048, np.uint32)
    for nb in range(nblk):
        lo, kind = nb * 2048, nb % 6
        if kind == 1: w[lo:lo + 2048] = 0xFFFFFFFF
        elif kind == 2: w[lo:lo + 2048] = rng.integers(0, 1 << 32, 2048, dtype=np.uint64).astype(np.uint32)
        elif kind == 4: w[lo + 100:lo + 900] = 0xFFFFFFFF; w[lo + 1500:lo + 1600] = 0xFFFFFFFF
        elif kind:
            for b in rng.integers(0, 65536, 40 if kind == 3 else 500): w[lo + (b >> 5)] |= np.uint32(1 << (b & 31))
    w[-25:] = 0
    return w


def spread_words(nblk=2000):
    w = np.zeros(nblk * 2048, np.uint32)
    for o in (5, 30000, 65000): w[np.arange(nblk) * 2048 + (o >> 5)] |= np.uint32(1 << (o & 31))
    return w


def vectors():
    yield "empty", bm.bit_import_u32(ctx, np.zeros(0, np.uint32))
    yield "mixed23", bm.bit_import_u32(ctx, mixed_words(), True)
    yield "dense40", bm.bvector.generate(ctx, SEED, 3, 6554, 40 * 65536 - 4321)
    yield "spread2000", bm.bit_import_u32(ctx, spread_words(), True)


def queries(rng, nbits, cnt, nq, ascending):
    q = np.concatenate([rng.integers(0, max(nbits, 1), size=max(nq - 2, 0)).astype(np.uint64), np.array([nbits, nbits + 70000], np.uint64)])[:nq]
    r = np.concatenate([rng.integers(1, cnt + 2, size=max(nq - 3, 0)).astype(np.uint64), np.array([0, cnt + 1, 2 ** 40], np.uint64)])[:nq]
    return (np.sort(q), np.sort(r)) if ascending else (q, r)


def ask(case, v, rs, info, nbits, cnt, sizes, **knobs):
    t = tune(QUERY_KEYS, {k: x for k, x in knobs.items() if k in QUERY_KEYS})
    if "rs_select_sel" in knobs: ctx.set_tuning("rs_select_sel", knobs["rs_select_sel"]); t += ",rs_select_sel=0"
    out = {"case": f"{case}/{t}", "info": info}
    for nq in sizes:
        q, r = queries(np.random.default_rng(nq), nbits, cnt, nq, knobs.get("rs_sorted_hint", 0))
        found, pos = v.select(r, rs)
        out[str(nq)] = {"rank": sha(v.rank(q, rs)), "pos": sha(pos), "found": sha(found)}
    print(json.dumps(out), flush=True)


for name, v in vectors():
    nbits, cnt = v.size(), v.count()
    for b in BUILDS:
        case = f"{name}/{tune(BUILD_KEYS, b)}"
        rs = v.build_rs_index()
        info = rs.info()
        assert rs.count() == cnt
        small = (1, 65535, 65536)
        if not cnt:                                        # the empty vector: the build alone (every stage returns early)
            print(json.dumps({"case": case, "info": info}), flush=True)
        elif info["select_offset_bits"]:
            # select lines serve whatever the other keys say; with rs_select_sel 0 at query time the index's other structures do
            for lanes in (0, 8): ask(case, v, rs, info, nbits, cnt, small, rs_lanes=lanes)
            for lanes, hint in itertools.product((0, 2, 4, 8), (0, 1)): ask(case, v, rs, info, nbits, cnt, small, rs_lanes=lanes, rs_sorted_hint=hint, rs_select_sel=0)
            ctx.set_tuning("rs_select_sel", b.get("rs_select_sel", -1))
        else:
            for lanes, sl, top, hint in itertools.product((0, 2, 4, 8), (0, 1, 2), (-1, 0, 1), (0, 1)):
                ask(case, v, rs, info, nbits, cnt, small, rs_lanes=lanes, rs_select_lines=sl, rs_select_top=top, rs_sorted_hint=hint)
            if info["has_lines"] and name in ("mixed23", "dense40") and "rs_sdir_shift" not in b:
                for top, hint in ((-1, 0), (-1, 1), (0, 0)): ask(case, v, rs, info, nbits, cnt, (1 << 22,), rs_select_top=top, rs_sorted_hint=hint)
        del rs
    tune(BUILD_KEYS, {}); tune(QUERY_KEYS, {})
    # the two callers of running_counts: to_indices, rank_compress / rank_decompress without an index (with one: its own counts)
    ids = v.to_indices()
    out = {"case": f"{name}/to_indices", "n": int(ids.size), "ids": sha(ids), "ids32": sha(v.to_indices(4)) if v.info()["nblocks"] <= 65536 else None}
    if cnt:
        rc, rs = bm.rank_compressor(ctx), v.build_rs_index()
        src = bm.bvector.from_indices(ctx, ids[::3], nbits)
        for tag, c in (("compress", rc.compress(v, src)), ("compress_rs", rc.compress_by_source(v, rs, src))):
            out[tag] = {"count": c.count(), "words": sha(c.to_words())}
            for tag2, d in ((tag + "/decompress", rc.decompress(v, c)), (tag + "/decompress_rs", rc.decompress(v, c, rs))):
                out[tag2] = {"count": d.count(), "words": sha(d.to_words())}
        del rs
    print(json.dumps(out), flush=True)
ctx.synchronize()
ctx.close()
