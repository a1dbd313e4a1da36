#!/usr/bin/env python3
"""Every path of the aggregator's list calls in bmx.hip (agg_or_choose / agg_and_sub_choose, the launch of each path, list_finish,
find_first_impl, or_target_run), once, at 64 blocks: what a launch / synchronise / copy / allocation count is taken over
(profiles/refactor_agg_lists).  Run it under `rocprofv3 --kernel-trace --hip-trace --stats -- python tools/agg_entries.py` against
two builds (BMX_LIB) and compare the tables; it prints one line per entry with the count and a hash of the words of the result.
TILE_AND_SORT_CALLS is the number of combine_or calls below that take the column-tile or the sort path."""
import hashlib, json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import bitmagic_amd as bm

SEED, NB = 0xB17A61C, 64 * 65536 - 77
TILE_AND_SORT_CALLS = 4                                   # or/tile and or/sort, each under both optimisation modes
ctx = bm.context(0)
agg = bm.aggregator(ctx)
out = {}


def pin(v):
    return [v.count(), hashlib.sha256(np.ascontiguousarray(v.to_words()).tobytes()).hexdigest()[:16]]


# 64 GAP-only vectors, each OR-ed with one common set (the AND results are not empty); 6 vectors of bit-blocks; one GAP vector
# without the common set (a SUB operand that leaves hits)
common = np.unique(np.random.default_rng(64).integers(0, NB, size=100, dtype=np.uint64))
cv = bm.bvector.from_indices(ctx, common, NB, optimize=True)
gap = [bm.bvector.bit_or(bm.bvector.generate(ctx, SEED, 100 + i, 66, NB), cv, bm.opt_compress) for i in range(64)]
assert all(g.info()["counts"][bm.BIT] == 0 and g.info()["counts"][bm.GAP] and g.info()["nblocks"] == 64 for g in gap)
dense = [bm.bvector.generate(ctx, SEED, 10 + i, dq, NB) for i, dq in enumerate((6554, 20000, 30000, 9000, 12000, 40000))]
other = bm.bvector.generate(ctx, SEED, 99, 66, NB)


def tuned(keys, call):
    for key, x in keys: ctx.set_tuning(key, x)
    try:
        return call()
    finally:
        for key, x in (("direct_cols", 384), ("or_rows", -1), ("coll_members", -1)): ctx.set_tuning(key, x)


def or_paths(paths):
    for opt in (False, True):
        agg.set_optimization(opt)
        for name, keys, some in paths:
            out[f"or/{name}/opt{int(opt)}"] = tuned(keys, lambda: pin(agg.combine_or(some)))
    agg.set_optimization(False)


# the OR paths no collection serves (none exists yet), then -- the 64 prepared in both roles -- the whole collection and 40 members
NO_DIRECT = ("direct_cols", 0)
or_paths((("none", (), []), ("direct", (), gap), ("rows", (NO_DIRECT, ("or_rows", 1)), gap), ("tile", (NO_DIRECT, ("or_rows", 0)), gap),
              ("sort", (NO_DIRECT,), gap[:63])))
assert ctx.pack_stats()["collections"] == 0
ctx.collection_prepare(gap, bm.ROLE_OR); ctx.collection_prepare(gap, bm.ROLE_AND)
or_paths((("collection", (NO_DIRECT,), gap), ("members", (NO_DIRECT, ("coll_members", 1)), gap[:40])))


def and_sub(a, s):
    t, any_ = agg.combine_and_sub(a, s)
    return pin(t) + [any_]


# the AND-SUB paths: empty AND list beside a SUB list, k_direct, the one-group pipeline, whole collections, members
out["and_sub/empty_and"] = and_sub([], dense[:2])
out["and_sub/direct"] = and_sub(dense[:3], dense[3:4])
out["and_sub/pipeline"] = tuned((NO_DIRECT,), lambda: and_sub(dense[:3], dense[3:4]))
out["and_sub/collections"] = tuned((NO_DIRECT,), lambda: and_sub(gap, []))
out["and_sub/members"] = tuned((NO_DIRECT, ("coll_members", 1)), lambda: and_sub(gap[:40], gap[48:56]))

# the first hit down both branches (the descriptor tables; the pipeline): with a hit, without one, ranged inside one block
mid = int(common[common.size // 2])
for cols, name in ((384, "direct"), (0, "pipeline")):
    ctx.set_tuning("direct_cols", cols)
    out[f"find_first/{name}/hit"] = list(agg.find_first_and_sub(gap[:3], [other]))
    out[f"find_first/{name}/none"] = list(agg.find_first_and_sub(gap[:2], gap[:1]))
    assert agg.set_range_hint(mid & ~0xFFFF, mid)                  # one block, partly covered
    out[f"find_first/{name}/ranged"] = list(agg.find_first_and_sub(gap[:3], [other]))
    agg.reset_range_hint()
ctx.set_tuning("direct_cols", 384)

# a results pipeline with an OR target that already holds bits, whole and under a one-block range hint
for name, hint in (("whole", None), ("hint", (mid & ~0xFFFF, mid))):
    pipe = bm.aggregator.pipeline(ctx, bm.agg_run_options(True, True, True))
    pipe.set_or_target(other)
    for a, s in ((gap[:3], [other]), (dense[:2], dense[2:3]), (gap[5:9], [])):
        ag = pipe.add()
        for v in a: ag.add(v, 0)
        for v in s: ag.add(v, 1)
    pipe.complete()
    if hint: assert agg.set_range_hint(*hint)
    agg.combine_and_sub(pipe)
    agg.reset_range_hint()
    out[f"results/{name}"] = pin(pipe.get_or_target()) + [[int(x) for x in pipe.get_bv_count_vector()]]

assert ctx.pack_stats()["collections"] == 2
ctx.synchronize()
for k, v in out.items():
    print(json.dumps({"entry": k, "result": v}))
ctx.close()
