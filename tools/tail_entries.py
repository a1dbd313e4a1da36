#!/usr/bin/env python3
"""Every entry that goes through the shared creation tail of bmx.hip (shard_window / layout_read / vec_all_null /
result_finish[_folded] / operand_list + direct_table), once, at a small size: what a launch / synchronise / copy count is taken
over (profiles/refactor_tail).  Run it under `rocprofv3 --kernel-trace --hip-trace --stats -- python tools/tail_entries.py`
against two builds (BMX_LIB) and compare the tables; it prints one line per entry with a figure that pins the result."""
import json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import bitmagic_amd as bm

SEED, NB = 0xB17A61C, 512 * 65536                       # 512 blocks: beyond the one-launch (k_direct) rule for >= 24 operands
ctx = bm.context(0)
agg = bm.aggregator(ctx)
rng = np.random.default_rng(5)
out = {}

ids = np.unique(rng.integers(0, NB, size=200_000, dtype=np.uint64))
out["from_indices_sorted"] = bm.bvector.from_indices(ctx, ids, NB, optimize=True).count()
out["from_indices_unsorted"] = bm.bvector.from_indices(ctx, rng.permutation(ids), NB, optimize=True).count()
out["from_indices_empty"] = bm.bvector.from_indices(ctx, np.zeros(0, np.uint64), NB).info()["counts"]
left = np.arange(0, NB - 4096, 4096, dtype=np.uint64)
pairs = np.stack([left, left + rng.integers(0, 2048, size=left.size).astype(np.uint64)], axis=1)
v_rng = bm.bvector.from_ranges(ctx, pairs, NB)
out["from_ranges_sorted"] = v_rng.count()
out["from_ranges_unsorted"] = bm.bvector.from_ranges(ctx, pairs[rng.permutation(left.size)], NB).count()
out["to_indices"] = int(v_rng.to_indices().size)
out["to_ranges"] = int(v_rng.to_ranges().shape[0])
out["bit_import_u32"] = bm.bit_import_u32(ctx, rng.integers(0, 1 << 32, size=NB // 32, dtype=np.uint32)).count()
dense = [bm.bvector.generate(ctx, SEED, 10 + i, 6554, NB) for i in range(30)]            # 10 %: bit-blocks
out["generate"] = dense[0].info()["counts"]

rc = bm.rank_compressor(ctx)
src = bm.bvector.bit_and(dense[0], dense[1])
for path in (0, 1):
    ctx.set_tuning("rankc_path", path)
    c = rc.compress(dense[0], src, optimize=True)
    out[f"rank_compress_path{path}"] = c.count()
    out[f"rank_decompress_path{path}"] = rc.decompress(dense[0], c, optimize=True).count()
    out[f"rank_compress_many_path{path}"] = [x.count() for x in rc.compress_many(dense[0], [src, dense[2]], optimize=True)]
ctx.set_tuning("rankc_path", -1)

out["bit_xor_x_x"] = bm.bvector.bit_xor(dense[0], dense[0]).info()["counts"]
out["bit_or"] = bm.bvector.bit_or(dense[0], dense[1]).count()
out["combine_or_direct"] = agg.combine_or(dense[:4]).count()                              # < 24 operands: k_direct
out["combine_or_general"] = agg.combine_or(dense).count()                                 # bit-blocks, 30 operands: k_or_sort + k_agg_or
sparse = [bm.bvector.generate(ctx, SEED, 100 + i, 13, NB) for i in range(64)]             # 0.02 %: GAP, <= 4.1 chunks per block
mid = [bm.bvector.generate(ctx, SEED, 200 + i, 66, NB) for i in range(64)]                # 0.1 %: GAP, longer blocks
out["combine_or_rows"] = agg.combine_or(sparse).count()                                   # k_agg_or_rows
out["combine_or_tiled"] = agg.combine_or(mid).count()                                     # k_agg_or_gap_tiled
ctx.collection_prepare(sparse, role=1)
out["combine_or_collection"] = agg.combine_or(sparse).count()                             # k_coll_apply, kinds folded
out["combine_or_members"] = agg.combine_or(sparse[:40]).count()                           # k_coll_members
t, any_ = agg.combine_and_sub([], dense[:2])
out["combine_and_sub_empty_and"] = [t.info()["counts"], any_]
t, any_ = agg.combine_and_sub(dense[:3], dense[3:4])
out["combine_and_sub"] = [t.count(), any_]
t, found = agg.combine_shift_right_and(dense[:4])
out["combine_shift_right_and"] = [t.count(), found]
t, found = agg.combine_shift_right_and([])
out["combine_shift_right_and_empty"] = [t.info()["counts"], found]
agg.set_compute_count(True)
agg.combine_shift_right_and(dense[:4])
out["combine_shift_right_and_count"] = agg.count()
agg.set_compute_count(False)
scan = bm.slice_scanner(ctx, dense[:8] + [None], size=NB)
out["find_gt"] = scan.find_gt(37).count()
out["find_range_count"] = scan.count(bm.CMP_RANGE, 5, 200)
ctx.synchronize()
for k, v in out.items():
    print(json.dumps({"entry": k, "result": v}))
