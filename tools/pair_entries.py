#!/usr/bin/env python3
"""Every path of the pairwise family (op2_plan / op2_launch / the result tails, count_op2_launch, bmx_i_count_async and
distance_pair_launch in bmx.hip), once, at small sizes: what a launch / synchronise / copy / allocation count is taken over
(profiles/refactor_pair).  Run it under `rocprofv3 --kernel-trace --hip-trace --stats -- python tools/pair_entries.py` against two
builds (BMX_LIB) and compare the tables; it prints one JSON line per case with info(), count() and a sha256 of to_words() and of
the block kinds, so that two builds can be held against each other line for line.  Block counts 0, 3, 2,047, 2,048 (the switch
to the long-vector kernels) and 2,100; operands of bit-blocks only, of bit-blocks with NULL / FULL holes and unequal lengths, and of
GAP blocks; the synchronous and the asynchronous entry; the tuning points that select another kernel."""
import hashlib, json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import bitmagic_amd as bm

SEED = 0xB17A61C
OPS = (("and", bm.AND), ("or", bm.OR), ("xor", bm.XOR), ("sub", bm.SUB))
KNOBS = (("op2_loop", -1), ("pair_stream", -1), ("op2_nt", 3), ("pair_loop", -1))
METRICS = (bm.COUNT_AND, bm.COUNT_XOR, bm.COUNT_OR, bm.COUNT_SUB_AB, bm.COUNT_SUB_BA, bm.COUNT_A, bm.COUNT_B)
ctx = bm.context(0)


def sha(x):
    return hashlib.sha256(np.ascontiguousarray(x).tobytes()).hexdigest()[:16]


def show(case, v):
    print(json.dumps({"case": case, "info": v.info(), "count": v.count(), "words": sha(v.to_words()), "kinds": sha(v.block_table()[0])}), flush=True)


def holes(rng, nblk, zero_every, ones_every):
    w = rng.integers(0, 1 << 32, nblk * 2048, dtype=np.uint64).astype(np.uint32)
    for b in range(nblk):
        if b % zero_every == 1: w[b * 2048:(b + 1) * 2048] = 0
        elif b % ones_every == 2: w[b * 2048:(b + 1) * 2048] = 0xFFFFFFFF
    return bm.bit_import_u32(ctx, w, True)


def operands(nblk):
    """-> {shape: (a, b)}"""
    if not nblk:
        return {"empty": (bm.bit_import_u32(ctx, np.zeros(0, np.uint32)), bm.bit_import_u32(ctx, np.zeros(0, np.uint32)))}
    rng = np.random.default_rng(nblk)
    gen = lambda v, dq: bm.bvector.generate(ctx, SEED, v, dq, nblk * 65536)
    return {"bits": (gen(1, 6554), gen(2, 20000)),                                   # bit-blocks only, equal length
            "holes": (holes(rng, nblk, 5, 7), holes(rng, max(nblk - 1, 1), 4, 9)),   # NULL / FULL holes, unequal lengths
            "gaps": (gen(3, 580), gen(4, 66))}                                       # GAP blocks (0.9 %: a few bit-blocks too; 0.1 %)


def sync_ops(tag, a, b, opt=bm.opt_none):
    for name, op in OPS:
        show(f"{tag}/sync/{name}", bm.bvector._op2(op, a, b, opt))


def async_ops(tag, a, b):
    # a chain over an unresolved operand, x op x over a vector and over an unresolved result, waits out of order
    r1 = bm.bvector.op2_async(bm.AND, a, b)
    r2 = bm.bvector.op2_async(bm.OR, r1, b)
    r3 = bm.bvector.op2_async(bm.SUB, a, r2)
    r4 = bm.bvector.op2_async(bm.XOR, r3, r1)
    same_v = [bm.bvector.op2_async(op, a, a) for _, op in OPS]
    same_p = [bm.bvector.op2_async(op, r4, r4) for _, op in OPS]
    for (name, _), p in reversed(list(zip(OPS, same_p))): show(f"{tag}/async/pending_{name}_itself", p.wait())
    show(f"{tag}/async/r4", r4.wait()); show(f"{tag}/async/r2", r2.wait()); show(f"{tag}/async/r1", r1.wait()); show(f"{tag}/async/r3", r3.wait())
    for (name, _), p in zip(OPS, same_v): show(f"{tag}/async/vector_{name}_itself", p.wait())


def counts(tag, a, b):
    out = {"case": f"{tag}/counts", "count_a": a.count(), "count_b": b.count(), "distance": bm.distance_operation(a, b, METRICS)}
    for name, f in (("and", bm.count_and), ("or", bm.count_or), ("xor", bm.count_xor), ("sub", bm.count_sub)): out[name] = f(a, b)
    print(json.dumps(out), flush=True)


def tuned(tag, a, b, **knobs):
    for k, x in knobs.items(): ctx.set_tuning(k, x)
    t = tag + "/" + ",".join(f"{k}={x}" for k, x in knobs.items())
    show(f"{t}/sync/and", bm.bvector.bit_and(a, b)); show(f"{t}/sync/xor", bm.bvector.bit_xor(a, b))
    show(f"{t}/async/sub", bm.bvector.op2_async(bm.SUB, a, b).wait())
    counts(t, a, b)
    for k, x in KNOBS: ctx.set_tuning(k, x)


for nblk in (0, 3, 2047, 2048, 2100):
    for shape, (a, b) in operands(nblk).items():
        tag = f"{shape}/{nblk}"
        sync_ops(tag, a, b)
        async_ops(tag, a, b)
        counts(tag, a, b)
        if nblk in (3, 2100) and shape != "bits":
            sync_ops(tag + "/opt_compress", a, b, bm.opt_compress)
        if nblk == 2100:
            for knobs in ({"op2_loop": 0}, {"op2_loop": 1}, {"pair_stream": 0}, {"op2_nt": 0}, {"pair_loop": 0}, {"pair_stream": 0, "op2_loop": 0}):
                tuned(tag, a, b, **knobs)
ctx.synchronize()
ctx.close()
