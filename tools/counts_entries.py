#!/usr/bin/env python3
"""Every kernel family a counts-only pipeline run can take (counts_plan in bmx.hip), once, at a small size, plus one run under
set_search_count_limit: what a launch / synchronise / copy count is taken over (profiles/refactor_plan).  Run it under
`rocprofv3 --kernel-trace --hip-trace --stats -- python tools/counts_entries.py` against two builds (BMX_LIB) and compare the
tables; it prints one line per case with describe(), launches() and the counts, so that a trace can be held against what the
library said it would launch."""
import json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bitmagic_amd as bm

SEED = 0xB17A61C
KNOBS = (("pipe_window", 0), ("pipe_split", -1), ("pipe_staged", -1), ("pipe_slots", 16), ("and_rows", -1), ("gap_count", -1), ("coll_members", -1))
ctx = bm.context(0)
agg = bm.aggregator(ctx)


def run(name, vecs, groups, rng=None, limit=None, **knobs):
    for k, x in KNOBS: ctx.set_tuning(k, knobs.get(k, x))
    pipe = bm.aggregator.pipeline(ctx)
    for a, s in groups:
        ag = pipe.add()
        for i in a: ag.add(vecs[i], 0)
        for i in s: ag.add(vecs[i], 1)
    if limit: pipe.set_search_count_limit(limit)
    pipe.complete()
    counts = agg._run_pipeline(pipe, *rng) if rng else agg.combine_and_sub(pipe)
    d, n = (pipe.describe(*rng), pipe.launches(*rng)) if rng else (pipe.describe(), pipe.launches())
    print(json.dumps({"case": name, "describe": d, "launches": n, "counts": [int(x) for x in counts]}), flush=True)


# 13 blocks of bit-blocks (10 %); with the sparse vector in a group the pipeline holds GAP blocks too: the general kernel
bits = [bm.bvector.generate(ctx, SEED, v, 6554, 13 * 65536, with_common=True) for v in range(19)]
mixed = bits + [bm.bvector.generate(ctx, SEED, 99, 66, 13 * 65536 + 5)]
few = [(list(range(5)), []), (list(range(8)), [8, 9]), ([0], [1]), (list(range(19)), [])]
few_mixed = few[:3] + [(list(range(20)), [])]
run("general", mixed, few_mixed)
run("general_windows", mixed, few_mixed, pipe_window=4)
run("bits", bits, few)
run("bits_windows", bits, few, pipe_window=4)
run("bits_one_launch", bits, few, pipe_window=-1)
run("split", bits, few, pipe_split=1)
run("staged8", bits, few, pipe_staged=1, pipe_slots=8)
run("staged16", bits, few, pipe_staged=1, pipe_slots=16)
run("empty_range", bits, few, rng=(3, 3))
run("search_limit", bits, few, limit=1000)
# 16 GAP-only vectors of 4 blocks (0.1 %)
gaps = [bm.bvector.generate(ctx, SEED, 100 + v, 66, 4 * 65536, with_common=True) for v in range(16)]
assert all(v.calc_stat()["bit_blocks"] == 0 and v.calc_stat()["gap_blocks"] for v in gaps)
some = [(list(range(16)), []), (list(range(0, 16, 2)), []), (list(range(3, 12)), [])]
run("and_rows", gaps, some, and_rows=1, pipe_split=0)
run("gapcount", gaps, some, gap_count=1, pipe_split=0)
ctx.collection_prepare(gaps, bm.ROLE_AND)
run("coll_whole", gaps, some[:1], pipe_split=0)
run("coll_members", gaps, some, coll_members=1, pipe_split=0)
for k, x in KNOBS: ctx.set_tuning(k, x)
ctx.synchronize()
ctx.close()
