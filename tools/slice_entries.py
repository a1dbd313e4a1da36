#!/usr/bin/env python3
"""Every entry that goes through the shared pieces of the bit-sliced search in bmx.hip (slice_column, the plane table,
vec_or_count_tail, first_hit_run, the two table forms of bmx_slice_eq_counts, range_counts_entry), once, at 64 blocks, each with
GAP-free and with GAP-holding planes: what a launch / synchronise / copy / allocation count is taken over
(profiles/refactor_slices).  Run it under `rocprofv3 --kernel-trace --hip-trace --stats -- python tools/slice_entries.py` against
two builds (BMX_LIB) and compare the tables; it prints one line per entry with a figure that pins the result."""
import hashlib, json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import bitmagic_amd as bm

SEED, NB = 0xB17A61C, 64 * 65536 - 77
ctx = bm.context(0)
agg = bm.aggregator(ctx)
out = {}


def sha(x):
    return hashlib.sha256(np.ascontiguousarray(x).tobytes()).hexdigest()[:16]


def pin(v):
    return [v.count(), sha(v.to_words())]


gen = lambda i, dq: bm.bvector.generate(ctx, SEED, i, dq, NB)
dense = [gen(i, dq) for i, dq in enumerate((6554, 20000, 3000, 9000, 12000, 30000, 6554, 800, 15000))]   # bit-blocks
sparse = [gen(20 + i, dq) for i, dq in enumerate((66, 200, 66, 13, 100, 66, 300, 66, 40))]              # GAP blocks
mixed = [dense[0], sparse[0], dense[1], sparse[1], dense[2], sparse[2], dense[3], sparse[3], dense[4]]
nn = gen(50, 60000)
COLUMNS = {"bits": dense, "gaps": mixed}

# find_first_and_sub down both branches (the descriptor tables; the pipeline), shift_right_and with a vector, a count, an empty list
for tag, v in COLUMNS.items():
    for cols, name in ((384, "direct"), (0, "pipeline")):
        ctx.set_tuning("direct_cols", cols)
        out[f"find_first/{tag}/{name}"] = list(agg.find_first_and_sub(v[:3], v[3:5]))
        out[f"find_first/{tag}/{name}/none"] = list(agg.find_first_and_sub(v[:2], v[:1]))
    ctx.set_tuning("direct_cols", 384)
    t, found = agg.combine_shift_right_and(v[:3])
    out[f"shift_right_and/{tag}"] = pin(t) + [found]
    agg.set_compute_count(True)
    agg.combine_shift_right_and(v[:3])
    out[f"shift_right_and/{tag}/count"] = agg.count()
    agg.set_compute_count(False)
t, found = agg.combine_shift_right_and([])
out["shift_right_and/empty"] = [t.info()["counts"], found]

# every predicate group of slice_compare, unsigned and signed, as a vector and as a count, under range_halves 0 and 1
PREDS = (("gt", bm.CMP_GT, 37, 0), ("le", bm.CMP_LE, 100, 0), ("range", bm.CMP_RANGE, 5, 200), ("eq", bm.CMP_EQ, 0, 0),
         ("zero", bm.CMP_ZERO, 0, 0), ("nonzero", bm.CMP_NONZERO, 0, 0))
SPREDS = (("gt_neg", bm.CMP_GT, -20, 0), ("lt_pos", bm.CMP_LT, 50, 0), ("range_neg", bm.CMP_RANGE, -90, -3), ("range_pos", bm.CMP_RANGE, 4, 77),
          ("range_across", bm.CMP_RANGE, -30, 30), ("eq_neg", bm.CMP_EQ, -5, 0), ("zero", bm.CMP_ZERO, 0, 0), ("nonzero", bm.CMP_NONZERO, 0, 0))
for tag, v in COLUMNS.items():
    planes = v[:3] + [None] + v[4:9]
    usc = bm.slice_scanner(ctx, planes, size=NB, not_null=nn)
    ssc = bm.slice_scanner(ctx, planes, size=NB, not_null=nn, signed=True)
    for halves in (0, 1):
        ctx.set_tuning("range_halves", halves)
        for sc, preds, kind in ((usc, PREDS, "u"), (ssc, SPREDS, "s")):
            for name, pred, v0, v1 in preds:
                out[f"compare/{tag}/{kind}/h{halves}/{name}"] = pin(sc._compare(pred, v0, v1)) + [sc.count(pred, v0, v1)]
        out[f"compare_stat/{tag}/h{halves}"] = list(usc.compare_stat(bm.CMP_RANGE, 5, 200))
    ctx.set_tuning("range_halves", 1)

    # mismatch as a vector, a count and the first; values and remap
    other = bm.slice_scanner(ctx, planes[:5] + [planes[6], planes[5]] + planes[7:], size=NB - 70000, not_null=gen(51, 61000))
    for proc, pname in ((bm.USE_NULL, "use_null"), (bm.NO_NULL, "no_null")):
        out[f"mismatch/{tag}/{pname}"] = (pin(bm.sparse_vector_find_mismatch(usc, other, proc)) + [bm.sparse_vector_count_mismatch(usc, other, proc)]
                                          + list(bm.sparse_vector_find_first_mismatch(usc, other, proc)))
    out[f"mismatch/{tag}/itself"] = list(bm.sparse_vector_find_first_mismatch(usc, usc, bm.NO_NULL))
    vals, rows = usc.values(sparse[4], rows=True)
    out[f"values/{tag}"] = [int(vals.size), sha(vals), sha(rows)]
    tr = bm.set2set_11_transform(ctx)
    out[f"remap/{tag}"] = pin(tr.remap(sparse[4], usc)) + [tr.n_rows]

    # eq_counts in both table forms (value 0, a value in the absent plane, one above the planes, duplicates)
    q = [0, 8, 1 << 9, 1 << 40, 5, 5] + list(range(1, 300, 3))
    for big in (0, 1):
        ctx.set_tuning("eq_big", big)
        out[f"eq_counts/{tag}/big{big}"] = sha(usc.find_eq_counts(q, method="transpose"))
    ctx.set_tuning("eq_big", -1)
    wide = bm.slice_scanner(ctx, planes + v[:4], size=NB, not_null=nn)   # 13 planes: 4,096 values can match
    many = list(range(1, 6000))                                      # ~3,000 of them unique and possible: two passes of the ordinal form
    for big in (0, -1):
        ctx.set_tuning("eq_big", big)
        out[f"eq_counts/{tag}/many/big{big}"] = sha(wide.find_eq_counts(many, method="transpose"))
    ctx.set_tuning("eq_big", -1)

    # eq_keys, the window smaller than the column (eqk_expand_kb) and the whole column
    strs = bm.str_scanner(ctx, planes, NB, nn)
    keys = np.array([[k & 255, k >> 8] for k in (0, 5, 1, 8, 247, 1 << 9, 5, 21, 300)], np.uint8)
    for kb in (256 * 1024, 128):                                     # 128 KiB over the 3 GAP planes of "gaps": 5 columns per window
        ctx.set_tuning("eqk_expand_kb", kb)
        cnt, first, found = strs.eq_keys(keys)
        out[f"eq_keys/{tag}/expand_kb{kb}"] = [cnt.tolist(), first.tolist(), found.tolist()]
    ctx.set_tuning("eqk_expand_kb", 256 * 1024)

    # range counts, unsigned and signed, one pass and several (rc_batch), the comparison path, the _stat entry
    lo, hi = [0, 10, 200, 30, 7], [9, 100, 255, 400, 7]
    slo, shi = [-100, -5, 3, -60, 0], [-7, 5, 90, -60, 0]
    for batch in (0, 2, -1):
        ctx.set_tuning("rc_batch", batch)
        out[f"range_counts/{tag}/u/batch{batch}"] = usc.find_range_counts(lo, hi).tolist()
        out[f"range_counts/{tag}/s/batch{batch}"] = ssc.find_range_counts(slo, shi).tolist()
        out[f"range_counts/{tag}/u/batch{batch}/one"] = usc.find_range_counts(lo[:1], hi[:1]).tolist()
        c, pb, nl = usc.range_counts_stat(lo, hi)
        out[f"range_counts_stat/{tag}/batch{batch}"] = [c.tolist(), pb, nl]
    ctx.set_tuning("rc_batch", 0)

ctx.synchronize()
for k, v in out.items():
    print(json.dumps({"entry": k, "result": v}))
ctx.close()
