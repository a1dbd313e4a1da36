"""GPU randomized differential stress test -- the analogue of StressTest / FillSetsRandomMethod
(tests/stress/t.cpp:917,11439): random block tables (every block independently NULL / FULL / bit / GAP with
random run structure, un-optimised representations included), random operations, compared with the oracle."""
import numpy as np
import pytest

import oracle

pytestmark = pytest.mark.gpu

import bitmagic_amd as bm  # noqa: E402


def _random_block(rng, kind):
    """-> 2048 uint32 words of one block of the requested flavour"""
    if kind == "zero":
        return np.zeros(2048, np.uint32)
    if kind == "ones":
        return np.full(2048, 0xFFFFFFFF, np.uint32)
    if kind == "dense":
        return rng.integers(0, 1 << 32, size=2048, dtype=np.uint64).astype(np.uint32)
    if kind == "sparse":
        w = np.zeros(2048, np.uint32)
        for p in rng.integers(0, 65536, size=int(rng.integers(1, 200))):
            w[p >> 5] |= np.uint32(1 << (int(p) & 31))
        return w
    if kind == "runs":                       # a few long runs: GAP with big interiors
        bits = np.zeros(65536, np.uint8)
        pos = np.sort(rng.integers(0, 65536, size=2 * int(rng.integers(1, 40))))
        for a, b in zip(pos[::2], pos[1::2]):
            bits[a:b + 1] = 1
        return np.packbits(bits, bitorder="little").view(np.uint32).copy()
    if kind == "antisparse":                 # almost all ones
        w = np.full(2048, 0xFFFFFFFF, np.uint32)
        for p in rng.integers(0, 65536, size=int(rng.integers(1, 100))):
            w[p >> 5] &= np.uint32(~(1 << (int(p) & 31)) & 0xFFFFFFFF)
        return w
    if kind == "edge":                       # bits at block / word / wave borders
        w = np.zeros(2048, np.uint32)
        for p in (0, 31, 32, 1023, 1024, 21824, 21825, 43648, 65535):
            if rng.integers(0, 2): w[p >> 5] |= np.uint32(1 << (p & 31))
        return w
    raise ValueError(kind)


KINDS = ["zero", "ones", "dense", "sparse", "runs", "antisparse", "edge"]


def _random_vector(rng, port, ctx, nblocks, optimize):
    words = np.concatenate([_random_block(rng, KINDS[int(rng.integers(0, len(KINDS)))]) for _ in range(nblocks)])
    pv = port.import_words(words, optimize, nblocks * 65536)
    if rng.integers(0, 2):                  # half of the vectors go through the host block-table upload
        k, o, b, g = pv.flatten()
        gv = bm.bvector.from_block_table(ctx, nblocks * 65536, k, o, b, g)
    else:
        gv = bm.bit_import_u32(ctx, words, optimize)
    return pv, gv


@pytest.mark.parametrize("seed", range(6))
def test_random_block_tables(ctx, port, seed, agg_path):
    rng = np.random.default_rng(1000 + seed)
    nvec = int(rng.integers(3, 14))
    vecs = [_random_vector(rng, port, ctx, int(rng.integers(1, 9)), bool(rng.integers(0, 2))) for _ in range(nvec)]
    pv = [v[0] for v in vecs]; gv = [v[1] for v in vecs]
    nwb = 9 * 2048
    agg = bm.aggregator(ctx)
    for v, g in zip(pv, gv):
        assert g.count() == v.count()
        assert (g.to_words(nwb) == v.to_words(nwb)).all()
    for _ in range(12):
        i, j = (int(x) for x in rng.integers(0, nvec, 2))
        op = int(rng.integers(0, 4)); opt = bm.opt_compress if rng.integers(0, 2) else bm.opt_none
        t = bm.bvector._op2(op, gv[i], gv[j], opt)
        e = port.op2(op, pv[i], pv[j], opt == bm.opt_compress)
        assert (t.to_words(nwb) == e.to_words(nwb)).all(), (seed, op, i, j)
        assert bm._count_op2(op, gv[i], gv[j]) == port.count_op2(op, pv[i], pv[j]) == e.count()
    groups = []
    for _ in range(10):
        na = int(rng.integers(1, nvec + 1)); ns = int(rng.integers(0, nvec))
        a = [int(x) for x in rng.integers(0, nvec, na)]; s = [int(x) for x in rng.integers(0, nvec, ns)]
        groups.append((a, s))
        t, any_ = agg.combine_and_sub([gv[k] for k in a], [gv[k] for k in s])
        e = port.agg_and_sub([pv[k] for k in a], [pv[k] for k in s])
        assert (t.to_words(nwb) == e.to_words(nwb)).all(), (seed, a, s)
        assert any_ == (e.count() > 0)
        f, idx = agg.find_first_and_sub([gv[k] for k in a], [gv[k] for k in s])
        pf, pidx = port.find_first_and_sub([pv[k] for k in a], [pv[k] for k in s])
        assert f == pf and (not f or idx == pidx), (seed, a, s, f, idx, pf, pidx)
        o = agg.combine_or([gv[k] for k in a + s])
        assert (o.to_words(nwb) == port.agg_or([pv[k] for k in a + s]).to_words(nwb)).all()
    exp = port.pipeline_counts([([pv[k] for k in a], [pv[k] for k in s]) for a, s in groups])
    for staged in (0, 1):
        ctx.set_tuning("pipe_staged", staged)
        try:
            pipe = bm.aggregator.pipeline(ctx)
            for a, s in groups:
                ag = pipe.add()
                for k in a: ag.add(gv[k], 0)
                for k in s: ag.add(gv[k], 1)
            pipe.complete()
            assert (agg.combine_and_sub(pipe) == exp).all(), (seed, staged)
        finally:
            ctx.set_tuning("pipe_staged", -1)
    # rank / select on a random member
    k = int(rng.integers(0, nvec))
    rs, prs = gv[k].build_rs_index(), port.rs_build(pv[k])
    nbits = pv[k].nbits
    q = rng.integers(0, nbits, size=400).astype(np.uint64)
    assert (gv[k].rank(q, rs) == prs.rank(q)).all()
    c = pv[k].count()
    r = rng.integers(0, c + 2, size=400).astype(np.uint64)
    found, pos = gv[k].select(r, rs)
    ppos, pfound = prs.select(r)
    assert (found == pfound).all() and (pos[found] == ppos[pfound]).all()
    bc, sub = rs.export(); pbc, psub = prs.export()
    assert (bc == pbc).all() and (sub == psub).all()


def test_error_behaviour(ctx):
    """status codes follow libbm's (lang-maps/libbm/include/libbm.h:28-35): BADARG = 2, RANGE = 3"""
    one = bm.bit_import_u32(ctx, np.array([5], np.uint32))
    with pytest.raises(bm.BmxError) as e:
        ctx.set_tuning("no_such_knob", 1)
    assert e.value.status == 2
    # malformed block tables are rejected, not trusted
    with pytest.raises(bm.BmxError) as e:
        bm.bvector.from_block_table(ctx, 65536, [bm.BIT], [3], np.zeros(2048, np.uint32), np.zeros(0, np.uint16))
    assert e.value.status == 3
    with pytest.raises(bm.BmxError) as e:                      # GAP block whose last run end is not 65535
        bm.bvector.from_block_table(ctx, 65536, [bm.GAP], [0], np.zeros(0, np.uint32), np.array([2 << 3, 100, 200], np.uint16))
    assert e.value.status == 3
    with pytest.raises(bm.BmxError) as e:
        bm.bvector.from_block_table(ctx, 65536, [7], [0], np.zeros(0, np.uint32), np.zeros(0, np.uint16))
    assert e.value.status == 2
    # run ends must be strictly ascending (checked on the device while the block is re-packed): an interior 65535, a
    # repeated end and a descending pair are all refused; so is a length beyond the top GAP level (1279 runs)
    good = np.array([(4 << 3), 10, 20, 30, 65535, 0, 0, 0], np.uint16)
    assert bm.bvector.from_block_table(ctx, 65536, [bm.GAP], [0], np.zeros(0, np.uint32), good).count() == 10 + 65505
    for bad in ([(4 << 3), 10, 65535, 30, 65535], [(4 << 3), 10, 10, 30, 65535], [(4 << 3), 30, 20, 40, 65535]):
        with pytest.raises(bm.BmxError) as e:
            bm.bvector.from_block_table(ctx, 65536, [bm.GAP], [0], np.zeros(0, np.uint32), np.array(bad + [0] * 3, np.uint16))
        assert e.value.status == 3, bad
    long_ = np.concatenate([[1280 << 3], np.arange(0, 2 * 1279, 2), [65535]]).astype(np.uint16)
    with pytest.raises(bm.BmxError) as e:
        bm.bvector.from_block_table(ctx, 65536, [bm.GAP], [0], np.zeros(0, np.uint32), long_)
    assert e.value.status == 3
    # two GAP blocks + a bit-block in one table: a bad SECOND block is found too, and nothing leaks (mem_used returns)
    used = ctx.mem_used()
    two = np.concatenate([good, np.array([(2 << 3), 500, 400, 0, 0, 0, 0, 0], np.uint16)])
    with pytest.raises(bm.BmxError):
        bm.bvector.from_block_table(ctx, 3 * 65536, [bm.GAP, bm.BIT, bm.GAP], [0, 0, 8], np.ones(2048, np.uint32), two)
    assert ctx.mem_used() == used
    pipe = bm.aggregator.pipeline(ctx)
    with pytest.raises(RuntimeError):
        bm.aggregator(ctx).combine_and_sub(pipe)               # not complete()
    ag = pipe.add(); ag.add(one, 0); pipe.complete()
    with pytest.raises(RuntimeError):
        pipe.add()                                             # no add() after complete()
    with pytest.raises(bm.BmxError) as e:                      # block range upside down
        bm.aggregator(ctx)._run_pipeline(pipe, 5, 2)
    assert e.value.status == 3
    # the allocator cache can be returned to the driver at any time
    before = ctx.mem_used(); ctx.trim(); assert ctx.mem_used() == before
    assert one.count() == 2


def test_degenerate_gap_blocks_and_unoptimized_tables(ctx, port):
    """vectors as an un-optimised reference container can hold them: GAP blocks that are
    all-zero / all-one (len 1), bit-blocks that are all-zero / all-one; treated by content, not by kind"""
    G0 = np.array([(1 << 3) | 0, 65535], np.uint16)              # all-zero GAP block
    G1 = np.array([(1 << 3) | 1, 65535], np.uint16)              # all-one GAP block
    G2 = np.array([(3 << 3) | 0, 99, 199, 65535], np.uint16)     # bits 100..199
    G3 = np.array([(2 << 3) | 1, 0, 65535], np.uint16)           # only bit 0
    gaps = np.concatenate([G0, G1, G2, G3])
    kinds = [bm.GAP, bm.GAP, bm.GAP, bm.GAP, bm.BIT, bm.BIT, bm.NULL, bm.FULL]
    offs = [0, 2, 4, 8, 0, 1, 0, 0]
    bits = np.concatenate([np.zeros(2048, np.uint32), np.full(2048, 0xFFFFFFFF, np.uint32)])
    nbits = 8 * 65536
    a = bm.bvector.from_block_table(ctx, nbits, kinds, offs, bits, gaps)
    pa = port.from_table(nbits, kinds, offs, bits, gaps)
    assert a.count() == pa.count() == 65536 + 100 + 1 + 65536 + 65536
    assert (a.to_words() == pa.to_words()).all()
    rng = np.random.default_rng(9)
    w = rng.integers(0, 1 << 32, size=8 * 2048, dtype=np.uint64).astype(np.uint32)
    b = bm.bit_import_u32(ctx, w, True); pb = port.import_words(w, True)
    agg = bm.aggregator(ctx)
    for op in range(4):
        for x, y, px, py in ((a, b, pa, pb), (b, a, pb, pa), (a, a, pa, pa)):
            for opt in (bm.opt_none, bm.opt_compress):
                t = bm.bvector._op2(op, x, y, opt)
                assert (t.to_words() == port.op2(op, px, py, opt == bm.opt_compress).to_words()).all(), (op, opt)
            assert bm._count_op2(op, x, y) == port.count_op2(op, px, py)
    t, _ = agg.combine_and_sub([a, b], [])
    assert (t.to_words() == port.agg_and_sub([pa, pb], []).to_words()).all()
    t, _ = agg.combine_and_sub([b], [a])
    assert (t.to_words() == port.agg_and_sub([pb], [pa]).to_words()).all()
    assert (agg.combine_or([a, b]).to_words() == port.agg_or([pa, pb]).to_words()).all()
    rs, prs = a.build_rs_index(), port.rs_build(pa)
    q = np.arange(0, nbits, 1237, dtype=np.uint64)
    assert (a.rank(q, rs) == prs.rank(q)).all()
    r = np.arange(1, pa.count() + 1, 997, dtype=np.uint64)
    f, p = a.select(r, rs); pp, pf = prs.select(r)
    assert f.all() and (p == pp).all()


def test_two_contexts_from_two_threads(port):
    """distinct contexts (one HIP stream each) may be driven concurrently from different host threads"""
    import threading
    nbits = 40 * 65536
    words = [port.gen_words(5150, v, 6554, nbits, with_common=True) for v in range(12)]
    exp = int(port.pipeline_counts([([port.import_words(w, True, nbits) for w in words], [])])[0])
    errors = []

    def work(tid):
        try:
            c = bm.context(0)
            vecs = [bm.bit_import_u32(c, w, True) for w in words]
            agg = bm.aggregator(c)
            for _ in range(20):
                pipe = bm.aggregator.pipeline(c)
                ag = pipe.add()
                for v in vecs: ag.add(v, 0)
                pipe.complete()
                got = int(agg.combine_and_sub(pipe)[0])
                t, _ = agg.combine_and_sub(vecs, [])
                if got != exp or t.count() != exp:
                    errors.append((tid, got, exp))
            del vecs
            c.close()
        except Exception as e:  # pragma: no cover
            errors.append((tid, repr(e)))

    th = [threading.Thread(target=work, args=(i,)) for i in range(3)]
    for t in th: t.start()
    for t in th: t.join()
    assert not errors, errors


@pytest.mark.parametrize("seed", range(40))
def test_block_kinds_follow_reference(ctx, port, seed):
    """REPRESENTATION parity on random block tables (tools/gpu_runs/soak.sh runs 400 of these): block kinds of the
    pairwise ops in both opt modes (copied bit / GAP blocks, GAP x GAP, computed blocks), of combine_and_sub, of
    combine_or with and without set_optimization, of pipeline results and the OR target, of shift-right-and.
    No whitelist: an all-ones GAP x GAP result is a 1-run GAP block here as in the reference (clone_gap_block)."""
    rng = np.random.default_rng(70000 + seed)
    nblk = int(rng.integers(1, 7)); nv = int(rng.integers(2, 7))
    vecs = [_random_vector(rng, port, ctx, nblk, bool(rng.integers(0, 2))) for _ in range(nv)]
    pv = [v[0] for v in vecs]; gv = [v[1] for v in vecs]
    for p, g in zip(pv, gv):
        assert g.block_table()[0].tolist() == p.flatten()[0].tolist()
    agg = bm.aggregator(ctx)
    for op in range(4):
        i, j = (int(x) for x in rng.integers(0, nv, 2))
        for oc in (True, False):
            kk = bm.bvector._op2(op, gv[i], gv[j], bm.opt_compress if oc else bm.opt_none).block_table()[0].tolist()
            ek = port.op2(op, pv[i], pv[j], oc).flatten()[0].tolist()
            assert kk == ek, (op, oc, i, j, kk, ek)
    na = int(rng.integers(1, nv + 1))
    t, _ = agg.combine_and_sub(gv[:na], gv[na:])
    assert t.block_table()[0].tolist() == port.agg_and_sub(pv[:na], pv[na:]).flatten()[0].tolist()
    for oc in (True, False):
        agg.set_optimization(oc)
        assert agg.combine_or(gv).block_table()[0].tolist() == port.agg_or(pv, oc).flatten()[0].tolist(), oc
        sel = [int(x) for x in rng.integers(0, nv, int(rng.integers(1, 12)))]
        t, f = agg.combine_shift_right_and([gv[k] for k in sel])
        e, ef = port.agg_shift_right_and([pv[k] for k in sel], oc, False)
        assert f == ef and t.block_table()[0].tolist()[:nblk] == e.flatten()[0].tolist()[:nblk]
    agg.set_optimization(False)


# the two entries of a materialised pairwise operation: bmx_op2, and bmx_op2_dev + bmx_pending_wait
_AND_ENTRIES = (("bit_and", lambda a, b: bm.bvector.bit_and(a, b)), ("op2_async", lambda a, b: bm.bvector.op2_async(bm.AND, a, b).wait()))


def test_result_memory_is_what_the_result_holds(ctx, port):
    """a materialised result keeps only what it holds: the full-size slab is transient.  AND of two vectors that meet in
    3 of 400 blocks: the result owns 3 bit-blocks (compacted), its download moves 3 blocks, content = oracle; a result
    that keeps 395 of 400 blocks stays in its slab (no second pass) and its download gathers the 395 live ones.  Both at 400
    blocks (a wave per column) and at 2,100 (past the 2,048-block switch to the persistent kernel; the transient slab is then
    17.2 MB), through the synchronous entry and through op2_async().wait().  Then operands of 2,100 GAP blocks (0.9 %: a few pass
    the GAP limit and are bit-blocks) whose AND holds a few bit-blocks and ~2,075 GAP blocks of 1 % of the operands' GAP words: the
    kernel lays the GAP results out into a slab sized at the operands' bound (9.6 MB), and the result keeps what it holds"""
    for nblk in (400, 2100):
        rng = np.random.default_rng(77)
        wa = np.zeros(nblk * 2048, np.uint32); wb = np.zeros(nblk * 2048, np.uint32)
        wa[:] = rng.integers(0, 1 << 32, wa.size, dtype=np.uint64).astype(np.uint32)
        for nb in (5, 200, nblk - 1):
            wb[nb * 2048:(nb + 1) * 2048] = rng.integers(0, 1 << 32, 2048, dtype=np.uint64).astype(np.uint32)
        a, b = bm.bit_import_u32(ctx, wa, True), bm.bit_import_u32(ctx, wb, True)
        pa, pb = port.import_words(wa, True, wa.size * 32), port.import_words(wb, True, wb.size * 32)
        # nearly full result: all but five blocks survive (b2 = all ones except five empty blocks)
        wb2 = np.full(nblk * 2048, 0xFFFFFFFF, np.uint32)
        for nb in (0, 7, 8, 123, nblk - 2):
            wb2[nb * 2048:(nb + 1) * 2048] = 0
        b2 = bm.bit_import_u32(ctx, wb2, True); pb2 = port.import_words(wb2, True, wb2.size * 32)
        e, e2 = port.op2(0, pa, pb, False), port.op2(0, pa, pb2, False)
        ew, ek, ew2 = e.to_words(), e.flatten()[0].tolist(), e2.to_words()
        for name, and_ in _AND_ENTRIES:
            t = None                                                          # (the other entry's result is not this one's credit)
            used = ctx.mem_used()
            t = and_(a, b)
            i = t.info()
            assert i["counts"][bm.BIT] == 3 and i["bit_slab_blocks"] == 3, (nblk, name, i)
            assert ctx.mem_used() - used < 3 * 8192 + 2 * (2 << 20), (nblk, name)   # not nblk x 8 KiB: three blocks + table (pool granules)
            k, o, bits, gaps = t.block_table()
            assert bits.size == 3 * 2048 and sorted(o[k == bm.BIT].tolist()) == [0, 1, 2], (nblk, name)
            assert (t.to_words() == ew).all() and k.tolist() == ek, (nblk, name)
            back = bm.bvector.from_block_table(ctx, nblk * 65536, k, o, bits, gaps)
            assert (back.to_words() == ew).all(), (nblk, name)
            t2 = and_(a, b2)
            i2 = t2.info()
            assert i2["counts"][bm.BIT] == nblk - 5 and i2["bit_slab_blocks"] == nblk - 5, (nblk, name, i2)
            k2, o2, bits2, gaps2 = t2.block_table()
            assert bits2.size == (nblk - 5) * 2048 and sorted(o2[k2 == bm.BIT].tolist()) == list(range(nblk - 5)), (nblk, name)
            back2 = bm.bvector.from_block_table(ctx, nblk * 65536, k2, o2, bits2, gaps2)
            assert (back2.to_words() == ew2).all() and (t2.to_words() == ew2).all(), (nblk, name)
            if nblk == 400 and name == "bit_and":
                keep = (a, b, t2, k2, o2, e2)
    # operands of GAP blocks, 2,100 of them: the kernel of either entry lays its GAP results out, the slab at the bound is trimmed
    nblk = 2100
    wga, wgb = (port.gen_words(77, v, 580, nblk * 65536) for v in (1, 2))
    ga, gb = bm.bit_import_u32(ctx, wga, True), bm.bit_import_u32(ctx, wgb, True)
    eg = port.op2(0, port.import_words(wga, True, nblk * 65536), port.import_words(wgb, True, nblk * 65536), False)
    egw, egk = eg.to_words(), eg.flatten()[0]
    live, operand_gap_words = int((egk == bm.BIT).sum()), ga.info()["gap_words"] + gb.info()["gap_words"]
    assert live == 13 and int((egk == bm.GAP).sum()) == 2075 and operand_gap_words > 4_500_000      # (the oracle's, for these seeds)
    redzone = 8192 if ctx.redzone_check()["enabled"] else 0
    for name, and_ in _AND_ENTRIES:
        t = and_(ga, gb)                                                    # (the context's scratch has grown to this shape)
        t = None
        used = ctx.mem_used()
        t = and_(ga, gb)
        grew = ctx.mem_used() - used
        i = t.info()
        print(name, "GAP case: grew", grew, "info", i)
        assert (t.block_table()[0] == egk).all() and (t.to_words() == egw).all(), name
        assert i["counts"][bm.BIT] == live and i["bit_slab_blocks"] == live and i["gap_words"] * 20 < operand_gap_words, (name, i)
        # what it holds, with the pool's best-fit slack (25 %) and one 2-MiB granule for each of the descriptor table, the bit slab,
        # the GAP slab and the ordinals; the GAP slab at the operands' bound alone is 9.6 MB
        assert grew < 1.25 * (live * 8192 + 2 * i["gap_words"] + 64 + 12 * nblk) + 4 * ((2 << 20) + redzone), (name, grew, i)
    a, b, t2, k2, o2, e2 = keep
    # a clone of a slab with unused slots keeps the ordinals; pipeline results over many groups stay small
    t3 = bm.bvector.bit_and(t2, t2)                                      # aliasing: block-for-block copy (src/bm.h:6191)
    assert (t3.to_words() == e2.to_words()).all() and t3.block_table()[1][k2 == bm.BIT].tolist() == o2[k2 == bm.BIT].tolist()
    pipe = bm.aggregator.pipeline(ctx, bm.agg_run_options(True, True))
    for _ in range(24):
        ag = pipe.add(); ag.add(a, 0); ag.add(b, 0)
    pipe.complete()
    used = ctx.mem_used()
    agg = bm.aggregator(ctx); agg.combine_and_sub(pipe)
    assert all(r.info()["bit_slab_blocks"] <= 3 for r in pipe.get_bv_res_vector())
    assert ctx.mem_used() - used < 24 * (3 * 8192 + (1 << 20)) + (8 << 20)   # 24 x 3 blocks, not 24 x 400


def test_randomized_soak_slices():
    """the randomized differential soaks (tools/soak_r04.py parts A-E: row kernel, collection members, long
    mixed pairwise operations, search limits, asynchronous chains; tools/soak_r05.py parts F-G: the AND rows kernel, per-group
    search limits; round 6: tools/soak_r06.py parts H-I: select lines, the search limit on the asynchronous counts entry) ran only under the builder's gpurun.  A bounded slice of each, fixed seeds, runs here: about a minute."""
    import subprocess, sys, os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for script, rounds in (("soak_r04.py", "4"), ("soak_r05.py", "14"), ("soak_r06.py", "8")):
        r = subprocess.run([sys.executable, os.path.join(root, "tools", script), rounds], capture_output=True, text=True, timeout=900, cwd=root)
        tail = (r.stdout + r.stderr)[-2000:]
        assert r.returncode == 0 and "done, failures: 0" in r.stdout, (script, tail)


_REDZONE_SCRIPT = r'''
import json, os, sys
sys.path.insert(0, os.getcwd())
import numpy as np
import bitmagic_amd as bm
import __graft_entry__ as g
g.smoke()                                            # pipeline counts, combine_and_sub, count_and, rs index + rank on a red-zone context
ctx = bm.context(0)
out = {"enabled": ctx.redzone_check()["enabled"]}
nbits = 40 * 65536 - 77
vs = [bm.bvector.generate(ctx, 99, i, dq, nbits) for i, dq in enumerate((6554, 655, 66, 30000, 200, 66, 66, 200))]
agg = bm.aggregator(ctx)
for op in ("bit_and", "bit_or", "bit_xor", "bit_sub"):
    r = getattr(bm.bvector, op)(vs[0], vs[1]); r.count(); r2 = getattr(bm.bvector, op)(vs[2], vs[4], bm.opt_compress); r2.count()
agg.combine_or(vs[2:]); agg.combine_and_sub(vs[4:6], [vs[6]])
ctx.collection_prepare(vs[4:], 1); agg.combine_or(vs[4:])
for v in (vs[0], vs[1], vs[2]):
    rs = v.build_rs_index(); n = rs.count()
    if n: v.select(np.arange(1, min(n, 5000) + 1, dtype=np.uint64), rs); v.rank(np.arange(0, nbits, 997, dtype=np.uint64), rs)
ctx.synchronize()
out["hits_after_workload"] = ctx.redzone_check()["hits"]
ctx.inject_failure(5, 0)                             # one byte written right behind a 1000-byte allocation
rep = ctx.redzone_check()
out["hits_after_self_test"] = rep["hits"]; out["report"] = rep["report"]
ctx.inject_failure(5, 7)                             # ... and behind a 1007-byte one: the zone starts at the next multiple of 16
out["hits_after_second"] = ctx.redzone_check()["hits"]
try:
    ctx.synchronize(); out["sync_after"] = "ok"
except bm.BmxError as e:
    out["sync_after"] = "error %d" % e.status
print("REDZONE " + json.dumps(out))
'''


def test_red_zone_allocator_catches_overruns_and_the_suite_is_clean():
    """a context created under BMX_DEBUG_REDZONE=1 surrounds every device allocation with canaries (in front, and
    from the end of the REQUESTED bytes to the end of the block) and verifies them at free / synchronize / destroy.  Here: the
    smoke workload + pairwise ops, aggregations, a collection, rs indexes (rank lines, select lines) run clean; a deliberate
    one-byte overrun IS caught and names the allocation; a slice of both soaks runs clean under the checker.  (The whole -m gpu
    suite + both soaks under the checker: profiles/r06_redzone/.)"""
    import json, os, subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, BMX_DEBUG_REDZONE="1")
    r = subprocess.run([sys.executable, "-c", _REDZONE_SCRIPT], capture_output=True, text=True, timeout=900, cwd=root, env=env)
    line = [l for l in r.stdout.splitlines() if l.startswith("REDZONE ")]
    assert r.returncode == 0 and line, (r.stdout + r.stderr)[-3000:]
    out = json.loads(line[0][8:])
    assert out["enabled"] and out["hits_after_workload"] == 0, out
    assert out["hits_after_self_test"] == 1 and out["hits_after_second"] == 2, out
    assert "BEHIND" in out["report"] and "1000 bytes" in out["report"] and "bmx.hip:" in out["report"], out
    assert out["sync_after"] == "ok"                   # (a damage is reported once: the zones were repainted)
    assert r.stderr.count("[bmx redzone] allocation") == 2, r.stderr[-2000:]
    for script, rounds in (("soak_r04.py", "2"), ("soak_r05.py", "6")):
        r = subprocess.run([sys.executable, os.path.join(root, "tools", script), rounds], capture_output=True, text=True, timeout=900, cwd=root, env=env)
        assert r.returncode == 0 and "done, failures: 0" in r.stdout and "[bmx redzone]" not in r.stderr, (script, (r.stdout + r.stderr)[-2000:])


def test_device_allocation_failures_come_back_as_status(port):
    """fault injection (bmx_debug_inject_failure kind 4): the k-th device allocation of a call fails; kind 6: it throws
    std::bad_alloc inside the library instead.  Whatever k, the call returns BMX_ERR_BADALLOC (or succeeds, if it allocates fewer
    than k + 1 times) -- never a crash, never a wrong answer -- the context keeps working, and what the failed call had allocated
    is given back."""
    import torch
    c = bm.context(0)
    nbits = 30 * 65536 - 5
    vs = [bm.bvector.generate(c, 5, i, dq, nbits) for i, dq in enumerate((6554, 655, 66, 66, 200, 66))]
    pv = [port.import_words(port.gen_words(5, i, dq, nbits), True, nbits) for i, dq in enumerate((6554, 655, 66, 66, 200, 66))]
    agg = bm.aggregator(c)
    exp_and = port.count_op2(0, pv[0], pv[1])
    exp_or = port.agg_or(pv[2:]).count()
    def pairwise(): return bm.bvector.bit_and(vs[0], vs[1]).count() == exp_and
    def combine_or(): return agg.combine_or(vs[2:]).count() == exp_or
    def rs_index():
        rs = vs[0].build_rs_index()
        return rs.count() == pv[0].count() and (vs[0].select(np.array([1, 77], np.uint64), rs)[1] == port.rs_build(pv[0]).select(np.array([1, 77], np.uint64))[0]).all()
    def prepare(): c.collection_prepare(vs[2:], 1); return agg.combine_or(vs[2:]).count() == exp_or
    def make_pipe(groups):
        pipe = bm.aggregator.pipeline(c)
        for a, s in groups:
            ag = pipe.add()
            for i in a: ag.add(vs[i], 0)
            for i in s: ag.add(vs[i], 1)
        return pipe
    def expect(groups): return [int(x) for x in port.pipeline_counts([([pv[i] for i in a], [pv[i] for i in s]) for a, s in groups])]
    def pipeline():
        pipe = make_pipe([([0, 1], [4])]); pipe.complete()
        return int(agg.combine_and_sub(pipe)[0]) == expect([([0, 1], [4])])[0]
    # 40 groups: the staged many-groups tables (pipeline_create uploads the plane masks)
    many = [([g % 2, 2 + g % 4], [2 + (g + 1) % 4]) for g in range(40)]
    exp_many = expect(many)
    def pipeline_staged():
        pipe = make_pipe(many); pipe.complete()
        return [int(x) for x in agg.combine_and_sub(pipe)] == exp_many
    # GAP-only groups under a search limit, through the asynchronous entry (limit_counts_run_dev)
    gap_groups = [([2, 3], []), ([2, 4], [5]), ([3, 4, 5], []), ([4], [2]), ([2, 5], [3]), ([5], [])]
    exp_gap, lim = expect(gap_groups), 5
    def pipeline_limit_dev():
        pipe = make_pipe(gap_groups); pipe.set_search_count_limit(lim); pipe.complete()
        d = torch.full((len(gap_groups),), -1, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        agg.run_counts_dev(pipe, d.data_ptr())
        c.synchronize()
        got = [int(x) for x in d.cpu().tolist()]
        return all(min(lim, t) <= g <= t for g, t in zip(got, exp_gap))
    # asynchronous results over GAP operands: a pending operand, the pending scratch and the wait's slab trim
    exp_async = port.count_op2(0, port.agg_or([pv[2], pv[3]]), pv[4])
    def op2_async():
        p1 = bm.bvector.op2_async(bm.OR, vs[2], vs[3])
        p2 = bm.bvector.op2_async(bm.AND, p1, vs[4])
        return p2.wait().count() == exp_async
    exp_and_sub = port.agg_and_sub([pv[0], pv[1]], [pv[4]]).count()
    def and_sub_materialised():
        t, _ = agg.combine_and_sub([vs[0], vs[1]], [vs[4]])
        return t.count() == exp_and_sub
    bt = vs[4].block_table()
    def upload_gap():
        u = bm.bvector.from_block_table(c, nbits, *bt)
        return u.count() == pv[4].count()
    exp_dist = np.array([[port.count_op2(0, pv[i], pv[j]) for j in (2, 3, 4)] for i in (2, 3, 4)], np.uint64)
    def distance_gap(): return (bm.distance_matrix([vs[2], vs[3], vs[4]])[0] == exp_dist).all()
    # ONE pipeline run again and again, its groups served by a prepared AND collection through the member directory: the member
    # table is built at the first run after the collections change (set_tuning bumps that at the end of a run that succeeded),
    # so a run whose table allocation failed is followed by a run of the same pipeline that must not use a table it does not have
    served_groups = [([2, 3], []), ([2, 4], []), ([3, 4, 5], []), ([4, 5], [])]
    exp_served, served = expect(served_groups), []
    def pipeline_coll_served():
        first = not served
        if first:
            c.collection_prepare([vs[i] for i in (2, 3, 4, 5)], bm.ROLE_AND)
            c.set_tuning("coll_members", 1)
            served.append(make_pipe(served_groups)); served[0].complete()
        ok = [int(x) for x in agg.combine_and_sub(served[0])] == exp_served
        if first: assert "k_coll_members" in served[0].describe()        # (the path this family is about)
        c.set_tuning("coll_members", 1)
        return ok
    # the bit-sliced scanner entries over two 8-plane columns: plane p of a column = vs[src[p]] (None: the plane is absent);
    # vs[2:] hold GAP blocks (the entries that walk raw planes expand them first).  Expected values: a numpy column rebuilt
    # from the same generated words, never the library
    def bits_of(i, dq):
        w = np.ascontiguousarray(port.gen_words(5, i, dq, nbits), np.uint32)
        return np.unpackbits(w.view(np.uint8), bitorder="little")[:nbits].astype(np.uint64)
    vbits = [bits_of(i, dq) for i, dq in enumerate((6554, 655, 66, 66, 200, 66))]
    def column(src):
        col = np.zeros(nbits, np.uint64)
        for p, i in enumerate(src):
            if i is not None: col |= vbits[i] << np.uint64(p)
        return col, [vs[i] if i is not None else None for i in src]
    col_a, planes_a = column([0, 2, 1, None, 3, 4, 5, 2])
    col_b, planes_b = column([0, 2, 1, None, 4, 3, 5, 2])
    sc_a, sc_b = bm.slice_scanner(c, planes_a, size=nbits), bm.slice_scanner(c, planes_b, size=nbits)
    exp_gt = np.flatnonzero(col_a > 37)
    def scan_gt_vector(): return np.array_equal(sc_a.find_gt(37).to_indices(), exp_gt)
    exp_range = int(((col_a >= 5) & (col_a <= 130)).sum())
    def scan_range_count(): return sc_a.count(bm.CMP_RANGE, 5, 130) == exp_range
    eq_vals = [0, 8, 1 << 9] + [int(v) for v in np.unique(col_a)[:40]] + [255, 247, 5, 5, 0, 1 << 40, 3]   # 0 twice, absent plane, above the planes
    exp_eq = [int((col_a == np.uint64(v)).sum()) for v in eq_vals]
    def scan_eq_counts(): return sc_a.find_eq_counts(eq_vals, method="transpose").tolist() == exp_eq
    key_vals = [0, 5, 1, 8, 247, 1 << 9, 5]                              # the empty key, absent plane, a bit past the planes, a duplicate
    keys = np.array([[v & 255, v >> 8] for v in key_vals], np.uint8)
    hits = [np.flatnonzero(col_a == np.uint64(v)) for v in key_vals]
    str_a = bm.str_scanner(c, planes_a, nbits)
    def scan_eq_keys():
        cnt, first, found = str_a.eq_keys(keys)
        return (cnt.tolist() == [h.size for h in hits] and found.tolist() == [int(h.size > 0) for h in hits]
                and first.tolist() == [int(h[0]) if h.size else 0 for h in hits])
    rc_lo, rc_hi = [0, 10, 200], [9, 100, 255]
    exp_rc = [int(((col_a >= lo) & (col_a <= hi)).sum()) for lo, hi in zip(rc_lo, rc_hi)]
    def scan_range_counts(): return sc_a.find_range_counts(rc_lo, rc_hi).tolist() == exp_rc
    exp_mm = np.flatnonzero(col_a != col_b)
    exp_image = np.unique(col_a[vbits[4] != 0])
    def scan_mismatch_remap():
        ok = np.array_equal(bm.sparse_vector_find_mismatch(sc_a, sc_b, bm.NO_NULL).to_indices(), exp_mm)
        return ok and np.array_equal(bm.set2set_11_transform(c).remap(vs[4], sc_a).to_indices(), exp_image)
    # the list calls of the aggregator down every path that does not go through k_direct: 64 GAP-only vectors (the smallest list
    # the row and the column-tile kernel take; 63 of them: the sort pass and k_agg_or<2>), each OR-ed with one common set so that
    # the AND results are not empty; in a context of its own (c2) the same 64 prepared as a collection in both roles: the whole
    # collection (kinds folded), 40 of its members, and the two AND-SUB forms of each.  A family names the context it runs in
    common = np.unique(np.random.default_rng(64).integers(0, nbits, size=100, dtype=np.uint64))
    cw = np.zeros(((nbits + 63) // 64) * 2, np.uint32)
    np.bitwise_or.at(cw, (common >> np.uint64(5)).astype(np.int64), np.uint32(1) << (common & np.uint64(31)).astype(np.uint32))
    p64 = [port.import_words(port.gen_words(5, 100 + i, 66, nbits) | cw, True, nbits) for i in range(64)]
    c2 = bm.context(0)
    agg2 = bm.aggregator(c2)
    def sparse64(cx):
        cv = bm.bvector.from_indices(cx, common, nbits, optimize=True)
        gv = [bm.bvector.bit_or(bm.bvector.generate(cx, 5, 100 + i, 66, nbits), cv, bm.opt_compress) for i in range(64)]
        info = [g.info() for g in gv]                    # what the selection reads: GAP blocks, no bit-block, 30 block columns
        assert all(i["counts"][bm.BIT] == 0 and i["counts"][bm.GAP] and i["nblocks"] == 30 for i in info)
        return gv
    g64, h64 = sparse64(c), sparse64(c2)
    c2.collection_prepare(h64, bm.ROLE_OR); c2.collection_prepare(h64, bm.ROLE_AND)
    assert c2.pack_stats()["collections"] == 2
    DEFAULTS = {"direct_cols": 384, "or_rows": -1, "coll_members": -1}
    def tuned(cx, keys, call):
        """call() under the tuning keys given; every one of them is put back, whatever came of the call"""
        for key, x in keys: cx.set_tuning(key, x)
        try:
            return call()
        finally:
            for key, _ in keys: cx.set_tuning(key, DEFAULTS[key])
    exp_or64, exp_or63, exp_or40 = port.agg_or(p64).count(), port.agg_or(p64[:63]).count(), port.agg_or(p64[:40]).count()
    exp_and64, exp_and40 = port.agg_and_sub(p64).count(), port.agg_and_sub(p64[:40], p64[48:56]).count()
    exp_first = port.find_first_and_sub(p64[:40], [pv[2]])
    assert exp_and64 >= common.size and exp_first[0]
    def or_rows(): return tuned(c, (("direct_cols", 0), ("or_rows", 1)), lambda: agg.combine_or(g64).count() == exp_or64)
    def or_tile(): return tuned(c, (("direct_cols", 0), ("or_rows", 0)), lambda: agg.combine_or(g64).count() == exp_or64)
    def or_sort(): return tuned(c, (("direct_cols", 0),), lambda: agg.combine_or(g64[:63]).count() == exp_or63)
    def or_coll(): return tuned(c2, (("direct_cols", 0),), lambda: agg2.combine_or(h64).count() == exp_or64)
    def or_members(): return tuned(c2, (("direct_cols", 0), ("coll_members", 1)), lambda: agg2.combine_or(h64[:40]).count() == exp_or40)
    def and_sub(a, s, exp):
        t, any_ = agg2.combine_and_sub(a, s)
        return t.count() == exp and any_ == (exp != 0)
    def and_coll(): return tuned(c2, (("direct_cols", 0),), lambda: and_sub(h64, [], exp_and64))
    def and_members(): return tuned(c2, (("direct_cols", 0), ("coll_members", 1)), lambda: and_sub(h64[:40], h64[48:56], exp_and40))
    def first_hit(): return tuple(agg.find_first_and_sub(g64[:40], [vs[2]])) == tuple(exp_first)
    def first_direct(): return tuned(c, (("direct_cols", 384),), first_hit)
    def first_pipeline(): return tuned(c, (("direct_cols", 0),), first_hit)
    for name, fn, *own in (("pairwise", pairwise), ("combine_or", combine_or), ("rs_index", rs_index), ("prepare", prepare), ("pipeline", pipeline),
                           ("pipeline_staged", pipeline_staged), ("pipeline_limit_dev", pipeline_limit_dev), ("op2_async", op2_async),
                           ("and_sub_materialised", and_sub_materialised), ("upload_gap", upload_gap), ("distance_gap", distance_gap),
                           ("pipeline_coll_served", pipeline_coll_served), ("scan_gt_vector", scan_gt_vector), ("scan_range_count", scan_range_count),
                           ("scan_eq_counts", scan_eq_counts), ("scan_eq_keys", scan_eq_keys), ("scan_range_counts", scan_range_counts),
                           ("scan_mismatch_remap", scan_mismatch_remap), ("or_rows", or_rows, c), ("or_tile", or_tile, c), ("or_sort", or_sort, c),
                           ("or_coll", or_coll, c2), ("or_members", or_members, c2), ("and_coll", and_coll, c2), ("and_members", and_members, c2),
                           ("first_direct", first_direct, c), ("first_pipeline", first_pipeline, c)):
        cx = own[0] if own else c
        assert fn(), name                                 # warm: pooled blocks, scratch sized
        cx.synchronize(); cx.trim()
        base, colls = cx.mem_used(), cx.pack_stats()["collections"]
        for kind in (4, 6):
            failed = 0
            for k in range(0, 40):
                cx.inject_failure(kind, k)
                try:
                    ok = fn()
                    assert ok, (name, kind, k)
                except bm.BmxError as e:
                    assert e.status == 1, (name, kind, k, str(e))
                    failed += 1
                finally:
                    cx.inject_failure(0, 0)
                cx.synchronize()
            assert fn(), (name, kind)
            cx.synchronize()
            assert failed >= 1, (name, kind)              # (every one of these calls allocates at least once)
        leaked = cx.mem_used() - base
        assert leaked <= (2 << 20), (name, leaked)        # (pool rounding of a fresh result may differ; a lost slab would be MBs per failure)
        if own: assert cx.pack_stats()["collections"] == colls, name      # (the list families: stays at what was prepared)
    h64.clear(); c2.close()
    c.close()
