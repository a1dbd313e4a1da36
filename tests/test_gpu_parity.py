"""GPU parity tests: the HIP path, driven through the C-ABI (ctypes binding of
include/bmx.h), against (1) the golden vectors the reference generated, (2) the CPU
oracle on seeded inputs, (3) size-independent properties at BASELINE.json sizes.
Bit-exact everywhere: all arithmetic is integer / bitwise."""
import numpy as np
import pytest

import oracle
from cases import (BM64_NVEC, bm64_build, bm64_queries, AGG_GROUPS, CASES, OR_SETS, PAIRS, SEED, make_inputs, rank_queries, select_queries, sha)

pytestmark = pytest.mark.gpu

import bitmagic_amd as bm  # noqa: E402


def _gap_masked(kinds, offs, gaps):
    g = gaps.copy()
    for k, o in zip(kinds, offs):
        if k == bm.GAP:
            g[o] &= 0xFFF9
    return g


def _compact_gaps(kinds, offs, gaps):
    """GAP blocks concatenated in block order (layout-independent view of the slab)"""
    out = []
    for k, o in zip(kinds, offs):
        if k == bm.GAP:
            n = (int(gaps[o]) >> 3) + 1
            blk = gaps[o:o + n].copy(); blk[0] &= 0xFFF9
            out.append(blk)
    return np.concatenate(out) if out else np.zeros(0, np.uint16)


def test_library_is_the_hip_one(ctx):
    assert bm.simd_version() == 950 and bm.device_count() >= 1


def test_generator_matches_oracle(ctx, port, golden):
    for dq, common, nbits in [(6554, False, 3 * 65536 + 17), (655, True, 2 * 65536), (66, False, 65536 + 5),
                              (32768, True, 70000), (65536, False, 1000), (0, False, 65536)]:
        v = bm.bvector.generate(ctx, SEED, 5, dq, nbits, with_common=common, optimize=False)
        exp = port.gen_words(SEED, 5, dq, nbits, with_common=common)
        got = v.to_words(exp.size)
        assert (got == exp).all(), (dq, common)
    # the normative known answers the reference-side fixture pins
    for k in golden["generator_kat"]:
        if k["w64"] < (1 << 20):
            nbits = (k["w64"] + 1) * 64
            v = bm.bvector.generate(ctx, SEED, k["vec"], k["dq"], nbits, optimize=False)
            w = v.to_words(nbits // 32)
            assert (int(w[-1]) << 32 | int(w[-2])) == k["word"]


@pytest.mark.parametrize("case", list(CASES))
def test_golden_case(ctx, port, golden, case, agg_path):
    g = golden["cases"][case]
    words, nbits = make_inputs(port, case)
    assert [sha(w) for w in words] == g["input_sha"]
    # (a) bit_import_u32 twin: classification + GAP conversion on the device
    vecs = [bm.bit_import_u32(ctx, w, True) for w in words]
    for v, w, kinds, gsha, cnt in zip(vecs, words, g["kinds"], g["gap_sha"], g["count"]):
        k, o, bits, gaps = v.block_table()
        assert k.tolist() == kinds
        assert sha(_compact_gaps(k, o, gaps)) == gsha or not gaps.size and gsha == sha(np.zeros(0, np.uint16))
        assert v.count() == cnt
        assert (v.to_words(w.size) == w).all()
    # (b) upload of a host block table (the oracle's flatten == walk of top_blocks_root())
    up = []
    for w in words:
        pv = port.import_words(w, True, nbits)
        k, o, bits, gaps = pv.flatten()
        u = bm.bvector.from_block_table(ctx, nbits, k, o, bits, gaps)
        assert (u.to_words(w.size) == w).all()
        up.append(u)
    nw = words[0].size
    nwb = ((nbits + 65535) // 65536) * 2048
    for (i, j) in PAIRS:
        for op, f, cf in [(0, bm.bvector.bit_and, bm.count_and), (1, bm.bvector.bit_or, bm.count_or),
                          (2, bm.bvector.bit_xor, bm.count_xor), (3, bm.bvector.bit_sub, bm.count_sub)]:
            e = g["op2"][f"{op}:{i}:{j}"]
            t = f(vecs[i], vecs[j])
            assert sha(t.to_words(nwb)) == e["sha"], (op, i, j)
            assert t.count() == e["count"]
            assert cf(vecs[i], up[j]) == e["count_op"]
            tc = f(up[i], vecs[j], bm.opt_compress)
            assert sha(tc.to_words(nwb)) == e["sha"]
            kk = tc.block_table()[0].tolist()
            # representation: identical to the reference, including the all-ones GAP x GAP result that
            # stays a 1-run GAP block (clone_gap_block, src/bmblocks.h:865-889)
            assert kk == e["kinds_opt"], (op, i, j, kk, e["kinds_opt"])
    agg = bm.aggregator(ctx)
    for e in g["agg_and_sub"]:
        t, any_ = agg.combine_and_sub([vecs[i] for i in e["and"]], [up[i] for i in e["sub"]])
        assert sha(t.to_words(nwb)) == e["sha"] and t.count() == e["count"]
        assert any_ == (e["count"] > 0)
        assert t.block_table()[0].tolist() == e["kinds"]
    for e in g["agg_or"]:
        t = agg.combine_or([vecs[i] for i in e["src"]])
        assert sha(t.to_words(nwb)) == e["sha"] and t.count() == e["count"]
        agg.set_optimization(True)
        assert agg.combine_or([vecs[i] for i in e["src"]]).block_table()[0].tolist() == e["kinds_opt"]
        agg.set_optimization(False)
    for e in g["shift_right_and"]:
        src = [(vecs if k % 2 else up)[i] for k, i in enumerate(e["src"])]
        agg.set_optimization(False)
        t, f = agg.combine_shift_right_and(src)
        assert sha(t.to_words(nwb)) == e["sha"] and t.count() == e["count"] and f == e["found"], e["src"]
        assert t.block_table()[0].tolist() == e["kinds"]
        agg.set_optimization(True)
        assert agg.combine_shift_right_and(src)[0].block_table()[0].tolist() == e["kinds_opt"]
        agg.set_optimization(False)
        ta, fa = agg.combine_shift_right_and(src, any=True)
        assert sha(ta.to_words(nwb)) == e["any_sha"] and ta.count() == e["any_count"] and fa == e["found"]
        agg.set_compute_count(True)
        none, fc = agg.combine_shift_right_and(src)
        assert none is None and agg.count() == e["count_mode"] and fc == e["found"]
        agg.set_compute_count(False)
    for e in g["find_first"]:
        f, idx = agg.find_first_and_sub([vecs[i] for i in e["and"]], [up[i] for i in e["sub"]])
        assert f == e["found"] and (not f or idx == e["idx"]), (e, f, idx)
    pipe = bm.aggregator.pipeline(ctx)
    for (a, s) in AGG_GROUPS:
        ag = pipe.add()
        for i in a: ag.add(vecs[i], 0)
        for i in s: ag.add(vecs[i], 1)
    pipe.complete()
    cnt = agg.combine_and_sub(pipe)
    assert [int(x) for x in cnt] == g["pipeline_counts"]
    assert [int(x) for x in pipe.get_bv_count_vector()] == g["pipeline_counts"]
    # pipeline::set_search_count_limit against what the REFERENCE returned under the same limit (golden "search_limit"): it
    # stops a group after the block where its count reached the limit, the library after the launch window -- both walk the
    # blocks in ascending order, so reference <= library <= true count, group by group ("can find more, cannot find less")
    for lim, ref_counts in g["search_limit"].items():
        pl = bm.aggregator.pipeline(ctx)
        for (a, s) in AGG_GROUPS:
            ag = pl.add()
            for i in a: ag.add(vecs[i], 0)
            for i in s: ag.add(vecs[i], 1)
        pl.set_search_count_limit(int(lim))
        pl.complete()
        got = [int(x) for x in agg.combine_and_sub(pl)]
        assert all(r <= x <= t for r, x, t in zip(ref_counts, got, g["pipeline_counts"])), (lim, ref_counts, got)
    # block-range shards add up (multi-GPU premise)
    nb = vecs[0].info()["nblocks"]
    parts = sum(agg._run_pipeline(pipe, a, b).astype(np.int64) for a, b in [(0, 1), (1, nb)])
    assert parts.tolist() == g["pipeline_counts"]
    # the other run options: result vectors + counts + OR target (pipeline<agg_opt_bvect_and_counts>)
    pr = g["pipeline_results"]
    for opt in (bm.agg_opt_bvect_and_counts, bm.agg_run_options(), bm.agg_opt_disable_bvects_and_counts):
        p2 = bm.aggregator.pipeline(ctx, opt)
        p2.set_or_target()
        for (a, s) in AGG_GROUPS:
            ag = p2.add()
            for i in a: ag.add(vecs[i], 0)
            for i in s: ag.add(up[i], 1)
        p2.complete()
        agg.combine_and_sub(p2)
        ort = p2.get_or_target()
        assert sha(ort.to_words(nwb)) == pr["or_target_sha"] and ort.count() == pr["or_target_count"]
        assert ort.block_table()[0].tolist() == pr["or_target_kinds"]
        if opt.is_make_results():
            res = p2.get_bv_res_vector()
            assert [r is not None for r in res] == pr["present"]
            assert [sha(r.to_words(nwb)) if r is not None else None for r in res] == pr["sha"]
            assert [r.block_table()[0].tolist() if r is not None else None for r in res] == pr["kinds"]
        if opt.is_compute_counts():
            assert [int(x) for x in p2.get_bv_count_vector()] == g["pipeline_counts"]
    # an OR target that already holds bits keeps them (combine_operation_block_or into the target, :1378-1389)
    p3 = bm.aggregator.pipeline(ctx, bm.agg_run_options())
    p3.set_or_target(vecs[5])
    ag = p3.add(); ag.add(vecs[0], 0); ag.add(vecs[1], 0)
    p3.complete(); agg.combine_and_sub(p3)
    exp = port.agg_or([port.import_words(words[5], True, nbits), port.agg_and_sub([port.import_words(words[0], True, nbits), port.import_words(words[1], True, nbits)])])
    assert (p3.get_or_target().to_words(nwb) == exp.to_words(nwb)).all()
    for e in g["rs"]:
        v = vecs[e["vec"]]
        rs = v.build_rs_index()
        assert rs.count() == e["count"]
        bc, sub = rs.export()
        assert bc.tolist() == e["bcount"][:len(bc)]
        assert [int(x) for x in sub] == e["sub_count"][:len(sub)]
        assert [int(x) for x in v.count_to(rank_queries(nbits), rs)] == e["rank"]
        found, pos = v.select(select_queries(e["count"]), rs)
        assert found.astype(int).tolist() == e["select_found"]
        assert [int(p) if f else 0 for p, f in zip(pos, found)] == e["select_pos"]
        rq, sq = rank_queries(nbits), select_queries(e["count"])
        assert [int(x) for x in v.count_range(rq[::7][:60], rq[3::7][:60], rs)] == e["count_range"]
        assert [int(x) for x in v.rank_corrected(rq[:120], rs)] == e["rank_corrected"]
        assert [int(x) for x in v.count_to_test(rq[:120], rs)] == e["count_to_test"]
        ff, fp = v.find_rank(sq[:40], rq[:40], rs)
        assert ff.astype(int).tolist() == e["find_rank_found"]
        assert [int(p) if f else 0 for p, f in zip(fp, ff)] == e["find_rank_pos"]


@pytest.mark.parametrize("dq,cdq,nvec", [(40, None, 9), (655, 655, 12), (6554, 6554, 40), (6554, None, 17),
                                         (32768, 20000, 33), (65500, None, 8)])
def test_differential_vs_oracle(ctx, port, dq, cdq, nvec, agg_path):
    """seeded random vectors incl. NULL/FULL blocks and ragged lengths; aggregator ladders over operand
    prefixes / suffixes as in StressTestAggregatorAND/OR (tests/stress/t.cpp:10811-11164)"""
    rng = np.random.default_rng(dq * 131 + nvec)
    nbits_max = 37 * 65536 + 1234
    pv, gv = [], []
    for v in range(nvec):
        nbits = nbits_max if v % 5 else nbits_max - 7 * 65536 - 99       # ragged
        w = port.gen_words(4242, v, dq, nbits)
        if cdq:
            w |= port.gen_words(4242, 0xFFFFFFFF, cdq, nbits)
            nw = (nbits + 31) // 32
            if nbits % 32: w[nw - 1] &= (1 << (nbits % 32)) - 1
            w[nw:] = 0
        for nb in range((w.size + 2047) // 2048):
            r = rng.integers(0, 24)
            if r == 0: w[nb * 2048:(nb + 1) * 2048] = 0
            elif r == 1 and (nb + 1) * 2048 <= (nbits // 32): w[nb * 2048:(nb + 1) * 2048] = 0xFFFFFFFF
        pv.append(port.import_words(w, True, w.size * 32))
        gv.append(bm.bit_import_u32(ctx, w, True))
        assert gv[-1].block_table()[0].tolist() == pv[-1].flatten()[0].tolist()
        assert gv[-1].count() == pv[-1].count()
    nwb = ((nbits_max + 65535) // 65536) * 2048
    agg = bm.aggregator(ctx)
    ladders = sorted(set([1, 2, 3, 5, 6, 7, 8, 9, nvec - 1, nvec]))
    groups = []
    for n in ladders:
        if n < 1 or n > nvec: continue
        groups.append((list(range(n)), []))
        groups.append((list(range(nvec - n, nvec)), list(range(0, max(0, nvec - n - 2), 3))))
    pipe = bm.aggregator.pipeline(ctx)
    for a, s in groups:
        ag = pipe.add()
        for i in a: ag.add(gv[i], 0)
        for i in s: ag.add(gv[i], 1)
    pipe.complete()
    got = agg.combine_and_sub(pipe)
    exp = port.pipeline_counts([([pv[i] for i in a], [pv[i] for i in s]) for a, s in groups])
    assert (got == exp).all(), (got, exp)
    for a, s in groups[::3]:
        t, _ = agg.combine_and_sub([gv[i] for i in a], [gv[i] for i in s])
        e = port.agg_and_sub([pv[i] for i in a], [pv[i] for i in s])
        assert (t.to_words(nwb) == e.to_words(nwb)).all()
        assert t.block_table()[0].tolist() == (e.flatten()[0].tolist() + [0] * 64)[:t.info()["nblocks"]]
        o = agg.combine_or([gv[i] for i in a + s])
        eo = port.agg_or([pv[i] for i in a + s])
        assert (o.to_words(nwb) == eo.to_words(nwb)).all()
    for i, j in [(0, 1), (1, 5), (2, nvec - 1)]:
        for op in range(4):
            t = bm.bvector._op2(op, gv[i], gv[j], bm.opt_none)
            e = port.op2(op, pv[i], pv[j])
            assert (t.to_words(nwb) == e.to_words(nwb)).all()
            assert t.block_table()[0].tolist() == (e.flatten()[0].tolist() + [0] * 64)[:t.info()["nblocks"]], (op, i, j)
            assert bm._count_op2(op, gv[i], gv[j]) == port.count_op2(op, pv[i], pv[j])
    # rank / select against the oracle on a mixed vector
    v, p = gv[1], pv[1]
    rs, prs = v.build_rs_index(), port.rs_build(p)
    q = rng.integers(0, nbits_max, size=5000).astype(np.uint64)
    assert (v.rank(q, rs) == prs.rank(q)).all()
    c = p.count()
    if c:
        r = np.concatenate([rng.integers(1, c + 1, size=5000).astype(np.uint64), np.array([1, c, 0, c + 1], np.uint64)])
        found, pos = v.select(r, rs)
        ppos, pfound = prs.select(r)
        assert (found == pfound).all() and (pos[found] == ppos[pfound]).all()


def test_kats_from_reference_tests(ctx, port, agg_path):
    """AggregatorTest known answers (tests/stress/t.cpp:10100-10152, 10318-10373) through the HIP path"""
    def mk(bits, n=3 * 65536, ranges=()):
        p = port.new(n)
        for b in bits: p.set_bit(b)
        for l, r in ranges: p.set_range(l, r)
        k, o, bs, gs = p.flatten()
        return bm.bvector.from_block_table(ctx, n, k, o, bs, gs)
    agg = bm.aggregator(ctx)
    a, b = mk([1, 2, 3]), mk([0, 4, 5])
    agg.add(a); agg.add(b)
    assert agg.combine_and().count() == 0
    t = agg.combine_or()
    assert t.count() == 6 and (t.to_words(1)[0] == 0b111111)
    assert agg.ag.arg_bv0 == []           # combine_or clears the arg-groups like the reference (:1110)
    agg.reset()
    c = mk([1, 2, 3, 4, 5, 70000])
    t, any_ = agg.combine_and_sub([c], [a])
    assert any_ and t.count() == 3
    f1, f2 = mk([], ranges=[(0, 65535)]), mk([], ranges=[(0, 2 * 65536 - 1)])
    assert agg.combine_or([f1, f2]).block_table()[0].tolist() == [bm.FULL, bm.FULL, bm.NULL]
    t, _ = agg.combine_and_sub([f1, f2], [])
    assert t.block_table()[0].tolist() == [bm.FULL, bm.NULL, bm.NULL] and t.count() == 65536
    # empty AND group => cleared target, any == false (src/bmaggregator.h:1170-1174)
    t, any_ = agg.combine_and_sub([], [a])
    assert not any_ and t.count() == 0
    # rank/select round trip on an all-ones vector (t.cpp:5005-5032)
    n = 4 * 65536
    ones = mk([], n=n, ranges=[(0, n - 1)])
    rs = ones.build_rs_index()
    q = np.arange(0, n, 997, dtype=np.uint64)
    assert (ones.rank(q, rs) == q + 1).all()
    found, pos = ones.select(q + 1, rs)
    assert found.all() and (pos == q).all()


def test_edge_cases(ctx):
    e = bm.bit_import_u32(ctx, np.zeros(0, np.uint32))
    assert e.count() == 0 and e.info()["nblocks"] == 0
    assert e.find() == (False, 0) and not e.any()
    # aliasing (src/bm.h:6191-6195, 5984-5988, 6081, 6412): AND / OR of a vector with itself copy it block for block
    # (an un-optimised all-zero bit-block stays a bit-block), XOR / SUB are empty
    raw = np.zeros(4 * 2048, np.uint32); raw[2048:4096] = 0xFFFFFFFF; raw[3 * 2048 + 5] = 77
    u = bm.bit_import_u32(ctx, raw, False)
    ku = u.block_table()[0].tolist()
    for fn in (bm.bvector.bit_and, bm.bvector.bit_or):
        for opt in (bm.opt_none, bm.opt_compress):
            c = fn(u, u, opt)
            assert c.block_table()[0].tolist() == ku and (c.to_words(raw.size) == raw).all() and c.count() == u.count()
    for fn in (bm.bvector.bit_xor, bm.bvector.bit_sub):
        z = fn(u, u)
        assert z.count() == 0 and set(z.block_table()[0].tolist()) == {bm.NULL} and z.info()["nblocks"] == 4
    w = np.zeros(3 * 2048, np.uint32); w[2 * 2048 + 17] = 1 << 9
    f = bm.bit_import_u32(ctx, w)
    assert f.find() == (True, 2 * 65536 + 17 * 32 + 9) and f.any()
    one = bm.bit_import_u32(ctx, np.array([1], np.uint32))
    assert one.count() == 1 and bm.count_and(one, e) == 0 and bm.count_or(one, e) == 1
    assert bm.bvector.bit_or(e, one).count() == 1 and bm.bvector.bit_sub(one, one).count() == 0
    agg = bm.aggregator(ctx)
    assert agg.combine_or([]).count() == 0
    other = bm.context(0)
    foreign = bm.bit_import_u32(other, np.array([1], np.uint32))
    with pytest.raises(bm.BmxError) as ei:
        bm.count_and(one, foreign)
    assert ei.value.status == 2
    del foreign
    other.close()


def test_full_size_pairwise_properties(ctx, port):
    """BASELINE config 2 size: two 1e9-bit vectors.  Size-independent identities + sampled blocks vs oracle."""
    nbits = 1_000_000_000
    for dq in (655, 6554, 32768):
        a = bm.bvector.generate(ctx, SEED, 1, dq, nbits)
        b = bm.bvector.generate(ctx, SEED, 2, dq, nbits)
        ca, cb = a.count(), b.count()
        c_and, c_or, c_xor, c_sub = bm.count_and(a, b), bm.count_or(a, b), bm.count_xor(a, b), bm.count_sub(a, b)
        assert c_and + c_sub == ca and c_or == ca + cb - c_and and c_xor == c_or - c_and
        p = dq / 65536
        assert abs(ca - p * nbits) < 8 * np.sqrt(nbits * p * (1 - p))
        t = bm.bvector.bit_and(a, b)
        assert t.count() == c_and
        x = bm.bvector.bit_xor(a, b, bm.opt_compress)
        assert x.count() == c_xor
        # idempotence / complement round trip:  (a XOR b) XOR b == a
        back = bm.bvector.bit_xor(x, b)
        assert bm.count_xor(back, a) == 0
        # sampled blocks against the oracle's generator + import
        for nb0 in (0, 7777, 15258):
            nw = min(2048, (nbits + 31) // 32 - nb0 * 2048)
            wa = port.gen_words(SEED, 1, dq, nbits, word_off=nb0 * 2048, nwords=nw)
            got = a.to_words((nb0 + 1) * 2048)[nb0 * 2048: nb0 * 2048 + nw]
            assert (got == wa).all()
        del t, x, back


@pytest.mark.parametrize("nblocks_x", [2048, 3001, 15259])
def test_pairwise_count_streaming_kernel(ctx, port, nblocks_x):
    """bm::count_* over two all-bit-block vectors takes the streaming kernel (a wave per stretch of columns, two
    columns in flight); every workgroup shape of it and the column-per-wave kernel (pair_stream 0) must return the
    same four counts; the AND count is also checked against the oracle on the same generated words"""
    nbits = nblocks_x * 65536 - 12345
    a = bm.bvector.generate(ctx, SEED + 9, 1, 20000, nbits)
    b = bm.bvector.generate(ctx, SEED + 9, 2, 30000, nbits)
    assert a.info()["counts"][bm.BIT] == nblocks_x and b.info()["counts"][bm.BIT] == nblocks_x
    try:
        ctx.set_tuning("pair_stream", 0)
        ref = [bm._count_op2(op, a, b) for op in range(4)]
        ca, cb = a.count(), b.count()                       # (count() of an all-bit vector takes the one-operand form of the same kernel)
        for ps, wgs in ((-1, 1), (2, 1), (2, 4), (4, 2), (8, 1), (4, 3)):
            ctx.set_tuning("pair_stream", ps); ctx.set_tuning("pair_wgs", wgs)
            assert [bm._count_op2(op, a, b) for op in range(4)] == ref, (ps, wgs)
            assert (a.count(), b.count()) == (ca, cb) and ca + cb == ref[0] + ref[1]
            assert bm._count_op2(bm.AND, b, a) == ref[0] and bm._count_op2(bm.SUB, b, a) == b.count() - ref[0]
    finally:
        ctx.set_tuning("pair_stream", -1); ctx.set_tuning("pair_wgs", 1); ctx.set_tuning("pipe_nt", 1)
    if nblocks_x <= 3001:
        wa = port.gen_words(SEED + 9, 1, 20000, nbits); wb = port.gen_words(SEED + 9, 2, 30000, nbits)
        assert ref[0] == int(np.unpackbits((wa & wb).view(np.uint8)).sum())
        assert ref[2] == int(np.unpackbits((wa ^ wb).view(np.uint8)).sum())


@pytest.mark.parametrize("nblocks_x", [2048, 3001])
def test_pairwise_materialised_streaming_kernel(ctx, port, nblocks_x):
    """bit_and/or/xor/sub over two all-bit-block vectors take the streaming kernel (k_op2_stream); every shape of it and the
    block-per-wave kernel (pair_stream 0) must produce the same words AND the same block kinds as the oracle: blocks
    that come out all-zero (-> NULL for AND / XOR / SUB) and all-ones (-> FULL for OR only) are planted"""
    rng = np.random.default_rng(nblocks_x)
    nw = nblocks_x * 2048 - 77
    wa = rng.integers(0, 1 << 32, size=nw, dtype=np.uint64).astype(np.uint32)
    wb = rng.integers(0, 1 << 32, size=nw, dtype=np.uint64).astype(np.uint32)
    B = 2048
    wa[3 * B:4 * B] = 0                                           # AND / SUB -> NULL, OR / XOR -> copy of b
    wb[5 * B:6 * B] = 0xFFFFFFFF                                  # OR -> FULL, SUB -> NULL
    wa[7 * B:8 * B] = wb[7 * B:8 * B]                             # XOR / SUB -> NULL
    wa[9 * B:10 * B] = ~wb[9 * B:10 * B]                          # AND -> NULL, OR / XOR -> all ones (XOR keeps a bit-block)
    wa[(nblocks_x - 1) * B:] = 0; wb[(nblocks_x - 1) * B:] = 0     # the short last block
    a = bm.bit_import_u32(ctx, wa, False); b = bm.bit_import_u32(ctx, wb, False)
    assert a.info()["counts"][bm.BIT] == nblocks_x and b.info()["counts"][bm.BIT] == nblocks_x
    pa = port.import_words(wa, False, nw * 32); pb = port.import_words(wb, False, nw * 32)
    fns = ((bm.bvector.bit_and, bm.AND), (bm.bvector.bit_or, bm.OR), (bm.bvector.bit_xor, bm.XOR), (bm.bvector.bit_sub, bm.SUB))
    try:
        for ps, wgs, nt in ((0, 1, 3), (-1, 1, 3), (-1, 2, 0), (-1, 3, 1), (-1, 8, 2)):
            ctx.set_tuning("pair_stream", ps); ctx.set_tuning("op2_wgs", wgs); ctx.set_tuning("op2_nt", nt)
            for fn, op in fns:
                t = fn(a, b)
                e = port.op2(op, pa, pb, 0)
                assert t.block_table()[0].tolist() == e.flatten()[0].tolist(), (ps, wgs, op)
                assert (t.to_words(nw) == e.to_words(nw)).all(), (ps, wgs, op)
                assert t.count() == e.count()
                st = t.calc_stat()
                assert st["bit_blocks"] == t.block_table()[0].tolist().count(bm.BIT)
                del t
    finally:
        ctx.set_tuning("pair_stream", -1); ctx.set_tuning("op2_wgs", 4); ctx.set_tuning("op2_nt", 3)


def test_rank_line_memory_policy(ctx, port):
    """build_rs_index lays a vector out as rank lines only where that costs <= 2 x the vector's own device bytes (rs_lines 1):
    a dense vector gets them, a sparse GAP vector (a configs[4] operand: 3.4 MB against 539 MB of lines) does not, and rank /
    select answer the same either way"""
    nbits = 600 * 65536 - 99
    dense = bm.bit_import_u32(ctx, port.gen_words(5, 1, 6554, nbits), True)
    sparse = bm.bit_import_u32(ctx, port.gen_words(5, 2, 13, nbits), True)
    assert sparse.calc_stat()["bit_blocks"] == 0
    rd, rsp = dense.build_rs_index(), sparse.build_rs_index()
    idn, isp = rd.info(), rsp.info()
    assert idn["has_lines"] and not isp["has_lines"]
    dev_bytes = lambda v: v.info()["gap_words"] * 2 + v.info()["nblocks"] * 8 + v.info()["counts"][bm.BIT] * 8192
    assert isp["bytes"] <= 1.2 * dev_bytes(sparse) + 600 * 300                # O(nblocks): running counts + two 128-byte rows per block
    assert idn["bytes"] - idn["select_lines_bytes"] <= 1.2 * dev_bytes(dense) + 600 * 300 + 16 * 600
    # select lines (round 6, rs_select_sel -1): 128 bytes per 60 (16-bit offsets) / 30 (32-bit) ones, where that is <= 2 x the vector
    # and its rank lines -- this 10 % vector takes the 16-bit form; the sparse one (13 ones per block: 60 of them span blocks) the 32-bit
    assert idn["select_offset_bits"] == 16 and idn["select_lines_bytes"] == (rd.count() + 59) // 60 * 128 <= 2 * 2.1 * dev_bytes(dense)
    assert isp["select_offset_bits"] == 32 and isp["select_lines_bytes"] == (rsp.count() + 29) // 30 * 128
    ps = port.import_words(port.gen_words(5, 2, 13, nbits), True, nbits)
    prs = port.rs_build(ps)
    rng = np.random.default_rng(3)
    q = rng.integers(0, nbits, 5000, dtype=np.uint64)
    assert (np.asarray(sparse.count_to(q, rsp)) == prs.rank(q)).all()
    r = rng.integers(1, prs.count() + 1, 5000, dtype=np.uint64)
    f, pos = sparse.select(r, rsp)
    assert np.asarray(f).all() and (np.asarray(pos) == prs.select(r)[0]).all()
    ctx.set_tuning("rs_lines", 2)                                                # forced: same answers through the lines
    try:
        rl = sparse.build_rs_index()
        assert rl.info()["has_lines"]
        assert (np.asarray(sparse.count_to(q, rl)) == prs.rank(q)).all()
        f2, pos2 = sparse.select(r, rl)
        assert np.asarray(f2).all() and (np.asarray(pos2) == np.asarray(pos)).all()
    finally:
        ctx.set_tuning("rs_lines", 1)


def test_rank_select_past_2_32_rank_lines(port):
    """a vector of 62.3 M blocks (4.08e12 bits: 69 rank lines per block would pass 2^32 line numbers, which are 32-bit): the
    index is built WITHOUT lines whatever rs_lines says (bmx_rs_build refuses them), stays O(nblocks), and rank / select over
    the mostly-NULL vector answer what the positions of its bits say (blocks of every kind far beyond bit 2^32 and 2^41)"""
    nblk_small = 6
    rng = np.random.default_rng(62)
    w = np.zeros(nblk_small * 2048, np.uint32)
    for b, n in ((0, 900), (1, 40), (3, 5), (5, 300)):                        # GAP blocks
        for q in rng.integers(0, 65536, size=n): w[b * 2048 + (int(q) >> 5)] |= np.uint32(1 << (int(q) & 31))
    w[2 * 2048:3 * 2048] = rng.integers(0, 1 << 32, size=2048, dtype=np.uint64).astype(np.uint32)   # a bit-block
    w[4 * 2048:5 * 2048] = 0xFFFFFFFF                                         # a FULL block
    small = port.import_words(w, True, nblk_small * 65536)
    k, o, b, g = small.flatten()
    assert sorted(set(k.tolist())) == [1, 2, 3]
    nblk = 62_300_000
    where = [0, 7, 31_000_000, 40_000_001, 62_200_123, nblk - 1]              # the six blocks, spread over the range
    kinds = np.zeros(nblk, np.uint8); offs = np.zeros(nblk, np.uint32)
    for i, nb in enumerate(where): kinds[nb] = k[i]; offs[nb] = o[i]
    bits = np.unpackbits(w.view(np.uint8), bitorder="little").reshape(nblk_small, 65536)
    pos = np.concatenate([np.flatnonzero(bits[i]).astype(np.uint64) + np.uint64(nb) * np.uint64(65536) for i, nb in enumerate(where)])
    assert (np.diff(pos.astype(np.int64)) > 0).all()
    c = bm.context(0)
    try:
        for mode in (1, 2):
            c.set_tuning("rs_lines", mode)
            v = bm.bvector.from_block_table(c, nblk * 65536, kinds, offs, b, g)
            assert v.count() == pos.size
            rs = v.build_rs_index()
            inf = rs.info()
            assert not inf["has_lines"] and rs.count() == pos.size
            assert inf["bytes"] <= nblk * 300 + (1 << 20)
            q = np.concatenate([rng.integers(0, nblk * 65536, size=4000, dtype=np.uint64), pos[::7], pos[::11] + np.uint64(1),
                                np.array([0, nblk * 65536 - 1, (1 << 32) - 1, 1 << 32, 1 << 41], np.uint64)])
            assert (np.asarray(v.count_to(q, rs)) == np.searchsorted(pos, q, side="right")).all()
            r = np.concatenate([rng.integers(1, pos.size + 1, size=4000, dtype=np.uint64), np.array([1, pos.size, pos.size + 1], np.uint64)])
            f, p_ = v.select(r, rs)
            f = np.asarray(f).astype(bool); p_ = np.asarray(p_)
            assert (f == (r <= pos.size)).all()
            assert (p_[f] == pos[(r[f] - 1).astype(np.int64)]).all()
            del rs, v
    finally:
        c.close()


def test_pipeline_search_count_limit(ctx, port):
    """pipeline::set_search_count_limit (src/bmaggregator.h:255, honoured at :1365: "can find more, cannot find less"): with
    limit L every group returns >= min(L, its true count) and <= its true count, and once every group has enough the remaining
    launch windows of block columns are not launched"""
    nbits = 3000 * 65536
    gv = [bm.bvector.generate(ctx, SEED, 40 + i, 6554, nbits, with_common=True) for i in range(6)]
    agg = bm.aggregator(ctx)
    def mk(limit=None):
        pipe = bm.aggregator.pipeline(ctx)
        for a, s in (([0, 1], [2]), ([0, 1, 2, 3], []), ([4], [5, 0])):
            ag = pipe.add()
            for i in a: ag.add(gv[i], 0)
            for i in s: ag.add(gv[i], 1)
        if limit is not None: pipe.set_search_count_limit(limit)
        pipe.complete()
        return pipe
    p0 = mk()
    full = [int(x) for x in agg.combine_and_sub(p0)]
    assert min(full) > 1000000 and p0.last_windows() == (1, 1)
    for limit in (1, 100, min(full) // 2, max(full) * 2):
        p = mk(limit)
        got = [int(x) for x in agg.combine_and_sub(p)]
        launched, planned = p.last_windows()
        assert all(min(limit, t) <= g <= t for g, t in zip(got, full)), (limit, got, full)
        if limit <= 100: assert launched == 1 and planned > 1, (limit, launched, planned)      # the first window already has enough for every group
        if limit == min(full) // 2: assert 1 < launched <= planned
        if limit > max(full): assert launched == planned and got == full
    p = mk(); p.set_search_count_limit(3)                                          # after complete()
    got = [int(x) for x in agg.combine_and_sub(p)]
    assert p.last_windows()[0] == 1 and all(3 <= g <= t for g, t in zip(got, full))


def test_full_size_256way_and_count(ctx, port):
    """BASELINE config 3: aggregator AND + COUNT over 256 x 1e9-bit vectors (correlated data set A).
    Checks: shard sums == total; sampled block columns equal the oracle run on the same
    generated inputs; monotonicity over operand prefixes."""
    nbits, nvec, dq = 1_000_000_000, 256, 6554
    vecs = [bm.bvector.generate(ctx, SEED, v, dq, nbits, with_common=True) for v in range(nvec)]
    agg = bm.aggregator(ctx)
    pipe = bm.aggregator.pipeline(ctx)
    for n in (256, 128, 2):
        ag = pipe.add()
        for v in vecs[:n]: ag.add(v, 0)
    pipe.complete()
    total = agg.combine_and_sub(pipe).astype(np.int64)
    assert total[0] <= total[1] <= total[2] and total[0] > 0
    nb = vecs[0].info()["nblocks"]
    assert nb == 15259
    cuts = [0, 1, 4000, 9999, nb]
    parts = sum(agg._run_pipeline(pipe, a, b).astype(np.int64) for a, b in zip(cuts[:-1], cuts[1:]))
    assert (parts == total).all()
    assert pipe.operand_bytes() == (256 + 128 + 2) * nb * 8192
    # sampled columns vs oracle
    for nb0 in (3, 15258):
        nw = min(2048, (nbits + 31) // 32 - nb0 * 2048)
        pvs = []
        for v in range(nvec):
            w = np.zeros((nb0 + 1) * 2048, np.uint32)
            w[nb0 * 2048: nb0 * 2048 + nw] = port.gen_words(SEED, v, dq, nbits, with_common=True, word_off=nb0 * 2048, nwords=nw)
            pvs.append(port.import_words(w, True))
        exp = port.pipeline_counts([(pvs[:256], []), (pvs[:128], []), (pvs[:2], [])], nb0, nb0 + 1)
        got = agg._run_pipeline(pipe, nb0, nb0 + 1)
        assert (got == exp).all(), (nb0, got, exp)
    # materialised combine_and over the same operands: windowed 640-thread launches (default), odd window sizes and the
    # single 256-thread launch must store the same vector; its population is the pipeline's count
    res = {}
    try:
        for name, win in (("windows", 0), ("one_launch", -1), ("odd", 1237)):
            ctx.set_tuning("pipe_window", win)
            res[name], any_ = agg.combine_and_sub(vecs[:128], [])
            assert any_ and res[name].count() == int(total[1]), name
    finally:
        ctx.set_tuning("pipe_window", 0)
    assert bm.count_xor(res["windows"], res["one_launch"]) == 0 and bm.count_xor(res["windows"], res["odd"]) == 0
    assert res["windows"].info()["counts"] == res["one_launch"].info()["counts"] == res["odd"].info()["counts"]
    t, _ = agg.combine_and_sub(vecs[:200], vecs[200:])           # SUB group of 56 operands that hold the common component: empty
    assert t.count() == 0


def _launch_shape_operands(ctx, port, tail_bits, nv=19):
    """nv vectors of 13 blocks (+ tail_bits: a 14th, GAP, block) with FULL and NULL blocks among the bit-blocks -> (device, oracle)"""
    nbits = 13 * 65536 + tail_bits
    words = []
    for v in range(nv):
        w = port.gen_words(777, v, 20000, nbits) | port.gen_words(777, 0xFFFFFFFF, 9000, nbits)
        if v % 7 == 3: w[2048:4096] = 0xFFFFFFFF                       # FULL block
        if v % 9 == 4: w[3 * 2048:4 * 2048] = 0                          # NULL block
        nw = (nbits + 31) // 32
        w[nw:] = 0; w[nw - 1] &= (1 << (nbits % 32)) - 1
        words.append(w)
    return [bm.bit_import_u32(ctx, w, True) for w in words], [port.import_words(w, True, w.size * 32) for w in words]


@pytest.mark.parametrize("tail_bits", [0, 5])
def test_launch_shape_knobs_do_not_change_results(ctx, port, tail_bits):
    """every tuning combination of the counts pipeline (slice size, batch size, NT, workgroup size, launch windows,
    XCD swizzle) x every operand count 1..19 (pipeline tail handling) x AND / AND-SUB groups.
    tail_bits 0: BIT / FULL / NULL blocks only -> the bit-only kernels k_pipe_counts_bits2<...> (the headline path);
    tail_bits 5: the last block is a GAP block -> the general kernel k_pipe_counts (the shape knobs must be harmless)."""
    nv = 19
    gv, pv = _launch_shape_operands(ctx, port, tail_bits)
    has_gap = any(g.calc_stat()["gap_blocks"] for g in gv)
    assert has_gap == (tail_bits != 0)
    assert sum(g.calc_stat()["full_blocks"] for g in gv) >= 2 and sum(g.calc_stat()["null_blocks"] for g in gv) >= 2
    groups = [(list(range(n)), []) for n in range(1, nv + 1)]
    groups += [(list(range(n)), list(range(n, min(nv, n + k)))) for n in (1, 2, 5, 8) for k in (1, 2, 3, 4, 5, 9)]
    exp = port.pipeline_counts([([pv[i] for i in a], [pv[i] for i in s]) for a, s in groups])
    pipe = bm.aggregator.pipeline(ctx)
    for a, s in groups:
        ag = pipe.add()
        for i in a: ag.add(gv[i], 0)
        for i in s: ag.add(gv[i], 1)
    pipe.complete()
    agg = bm.aggregator(ctx)
    try:
        # every launch shape the default build carries (slice size x unroll x nt x workgroup size) x launch windows
        shapes = [(8, 4, 1, wg, win) for wg in (256, 384, 512, 640, 768) for win in (0, -1, 3)]
        shapes += [(rows, u, 1, 256, win) for rows in (4, 2, 1) for u in (4, 8) for win in (0, -1)]
        shapes += [(rows, 4, 0, 256, 0) for rows in (8, 4, 2, 1)] + [(8, 4, 0, 512, 0), (0, 0, 0, 0, 0), (0, 0, 1, 0, 0), (0, 0, 1, 0, 2)]
        ctx.set_tuning("pipe_staged", 0)                        # many groups over few vectors would pick the LDS-staged kernel
        for rows, u, nt, wg, win in shapes:
            for swz in (1, 0):
                for k, x in (("pipe_unroll", u), ("pipe_rows", rows), ("pipe_nt", nt), ("pipe_wg", wg), ("pipe_window", win), ("xcd_swizzle", swz)):
                    ctx.set_tuning(k, x)
                got = agg.combine_and_sub(pipe)
                assert (got == exp).all(), (rows, u, nt, wg, win, swz)
                nb = gv[0].info()["nblocks"]
                parts = sum(agg._run_pipeline(pipe, a, b).astype(np.int64) for a, b in [(0, 3), (3, 4), (4, nb)])
                assert (parts == exp.astype(np.int64)).all(), (rows, u, nt, wg, win, swz)
        ctx.set_tuning("pipe_wg", 192)                          # a shape only the tuning build carries: refused, not mis-launched
        if not has_gap:
            assert "k_pipe_counts_bits2<" in pipe.describe()
            with pytest.raises(bm.BmxError):
                agg.combine_and_sub(pipe)
        else:
            assert "k_pipe_counts<" in pipe.describe()
        for k, x in (("pipe_unroll", 0), ("pipe_rows", 0), ("pipe_nt", 1), ("pipe_wg", 0), ("pipe_window", 0), ("xcd_swizzle", 1)):
            ctx.set_tuning(k, x)
        # operand lists split over the waves of a workgroup (few columns, long lists): counts and materialised results
        for split in (1, 0, -1):
            ctx.set_tuning("pipe_split", split)
            assert (agg.combine_and_sub(pipe) == exp).all(), ("split", split)
            nb = gv[0].info()["nblocks"]
            parts = sum(agg._run_pipeline(pipe, a, b).astype(np.int64) for a, b in [(0, 2), (2, nb)])
            assert (parts == exp.astype(np.int64)).all(), ("split", split)
            for a, s_ in groups[::5]:
                t, _ = agg.combine_and_sub([gv[i] for i in a], [gv[i] for i in s_])
                e = port.agg_and_sub([pv[i] for i in a], [pv[i] for i in s_])
                assert (t.to_words(14 * 2048) == e.to_words(14 * 2048)).all() and t.block_table()[0].tolist() == e.flatten()[0].tolist()
        assert "k_pipe_split" in (ctx.set_tuning("pipe_split", 1) or pipe.describe())
        ctx.set_tuning("pipe_split", -1)
        # LDS-staged many-groups kernel forced on (19 planes = 2 chunks, FULL / NULL planes, AND-SUB masks)
        for swz, slots in ((0, 16), (1, 16), (1, 8)):
            ctx.set_tuning("pipe_staged", 1); ctx.set_tuning("xcd_swizzle", swz); ctx.set_tuning("pipe_slots", slots)
            got = agg.combine_and_sub(pipe)
            assert (got == exp).all(), ("staged", swz, got, exp)
            nb = gv[0].info()["nblocks"]
            parts = sum(agg._run_pipeline(pipe, a, b).astype(np.int64) for a, b in [(0, 5), (5, nb)])
            assert (parts == exp.astype(np.int64)).all()
    finally:
        for k, x in (("pipe_unroll", 0), ("pipe_rows", 0), ("pipe_nt", 1), ("pipe_wg", 0), ("pipe_window", 0), ("xcd_swizzle", 1),
                     ("pipe_staged", -1), ("pipe_slots", 16), ("pipe_split", -1)):
            ctx.set_tuning(k, x)
    # the materialising twins use the same fold: every prefix, AND-SUB and OR
    for a, s in groups[::4]:
        t, _ = agg.combine_and_sub([gv[i] for i in a], [gv[i] for i in s])
        e = port.agg_and_sub([pv[i] for i in a], [pv[i] for i in s])
        assert (t.to_words(14 * 2048) == e.to_words(14 * 2048)).all()
        o = agg.combine_or([gv[i] for i in a + s])
        assert (o.to_words(14 * 2048) == port.agg_or([pv[i] for i in a + s]).to_words(14 * 2048)).all()


# what pipe.describe() printed for the cases of test_describe_is_the_launch_plan BEFORE the launch plan became one function
# (taken from that library, not from the one under test), and the launches each line names.  One line differs on purpose:
# the general kernel under pipe_window > 0 printed "k_pipe_counts<4> x 1 launch" while it launched four windows.
_PLAN_TEXT = {
    "general": ("k_pipe_counts<4> x 1 launch", 1),
    "general_windows": ("k_pipe_counts<4> x 4 launches of <= 4 columns", 4),
    "bits": ("k_pipe_counts_bits2<8,true,256,1> x 1 launch of <= 13 columns", 1),
    "bits_windows": ("k_pipe_counts_bits2<8,true,256,1> x 4 launches of <= 4 columns", 4),
    "bits_one_launch": ("k_pipe_counts_bits2<8,true,256,1> x 1 launch of <= 13 columns", 1),
    "split": ("k_pipe_split<2,8> x 1 launch, 52 workgroups", 1),
    "staged8": ("k_pipe_counts_staged<8> x 1 launch, 13 workgroups", 1),
    "staged16": ("k_pipe_counts_staged<16> x 1 launch, 13 workgroups", 1),
    "empty_range": ("k_pipe_counts_bits2<8,true,256,1> x 1 launch of <= 0 columns", 1),
    "and_rows": ("k_agg_and_rows<COUNT,256,3> x 1 launch, 12 workgroups", 1),
    "gapcount": ("k_pipe_counts_gapcount x 1 launch, 12 workgroups", 1),
    "coll_whole": ("k_coll_apply<AND_COUNT,512> x 1 launch, 4 workgroups (packed collection of the operand set)", 1),
    "coll_members": ("k_coll_members<AND_COUNT> x 1 launch, a wave per (column, group): 4 x 3 items (members of a packed collection)", 1),
}
_PLAN_KNOBS = (("pipe_window", 0), ("pipe_split", -1), ("pipe_staged", -1), ("pipe_slots", 16), ("and_rows", -1), ("gap_count", -1), ("coll_members", -1))


def _plan_cases(ctx, port):
    """every kernel family of a counts-only run, once: yields (name, pipeline, oracle groups, block range or None) with the
    case's tuning keys in force.  Operands: the launch-shape vectors (13 bit-blocks; + a GAP block for the general kernel) and 16
    GAP-only vectors of 4 blocks; a few arg-groups each."""
    def make(gv, pv, groups, **knobs):
        for k, x in _PLAN_KNOBS: ctx.set_tuning(k, knobs.get(k, x))
        pipe = bm.aggregator.pipeline(ctx)
        for a, s in groups:
            ag = pipe.add()
            for i in a: ag.add(gv[i], 0)
            for i in s: ag.add(gv[i], 1)
        pipe.complete()                                        # (the staged tables of a few-group pipeline exist only under pipe_staged 1)
        return pipe, [([pv[i] for i in a], [pv[i] for i in s]) for a, s in groups]
    few = [(list(range(5)), []), (list(range(8)), [8, 9]), ([0], [1]), (list(range(19)), [])]
    bits, mixed = _launch_shape_operands(ctx, port, 0), _launch_shape_operands(ctx, port, 5)
    assert not any(g.calc_stat()["gap_blocks"] for g in bits[0]) and any(g.calc_stat()["gap_blocks"] for g in mixed[0])
    yield ("general",) + make(*mixed, few) + (None,)
    yield ("general_windows",) + make(*mixed, few, pipe_window=4) + (None,)
    yield ("bits",) + make(*bits, few) + (None,)
    yield ("bits_windows",) + make(*bits, few, pipe_window=4) + (None,)
    yield ("bits_one_launch",) + make(*bits, few, pipe_window=-1) + (None,)
    yield ("split",) + make(*bits, few, pipe_split=1) + (None,)
    yield ("staged8",) + make(*bits, few, pipe_staged=1, pipe_slots=8) + (None,)
    yield ("staged16",) + make(*bits, few, pipe_staged=1, pipe_slots=16) + (None,)
    yield ("empty_range",) + make(*bits, few) + ((3, 3),)
    nbits = 4 * 65536
    common = port.gen_words(777, 0xFFFFFFFF, 40, nbits)
    words = [port.gen_words(777, 100 + v, (30, 120, 300)[v % 3], nbits) | common for v in range(16)]
    gaps = [bm.bit_import_u32(ctx, w, True) for w in words], [port.import_words(w, True, w.size * 32) for w in words]
    assert all(v.calc_stat()["bit_blocks"] == 0 and v.calc_stat()["gap_blocks"] for v in gaps[0]), "the case must stay GAP-only"
    some = [(list(range(16)), []), (list(range(0, 16, 2)), []), (list(range(3, 12)), [])]
    yield ("and_rows",) + make(*gaps, some, and_rows=1, pipe_split=0) + (None,)
    yield ("gapcount",) + make(*gaps, some, gap_count=1, pipe_split=0) + (None,)
    ctx.collection_prepare(gaps[0], bm.ROLE_AND)               # (goes with its vectors)
    yield ("coll_whole",) + make(*gaps, some[:1], pipe_split=0) + (None,)
    yield ("coll_members",) + make(*gaps, some, coll_members=1, pipe_split=0) + (None,)


def test_describe_is_the_launch_plan(ctx, port):
    """pipe.describe() / pipe.launches() are the plan the counts run launches (counts_plan in bmx.hip), not a second derivation
    of it: for every kernel family the counts equal the oracle's, the text is what the library printed before the two were
    joined (_PLAN_TEXT) and launches() is the number of launches that text names -- several where pipe_window cuts the 13 / 14
    columns into windows of 4, the general kernel included."""
    agg = bm.aggregator(ctx)
    seen = []
    try:
        for name, pipe, groups, rng in _plan_cases(ctx, port):
            if rng is None: got, exp = agg.combine_and_sub(pipe), port.pipeline_counts(groups)
            else: got, exp = agg._run_pipeline(pipe, *rng), port.pipeline_counts(groups, *rng)
            text, launches = _PLAN_TEXT[name]
            d = pipe.describe(*rng) if rng else pipe.describe()       # (after the run: a collection serves a pipeline from its first run on)
            n = pipe.launches(*rng) if rng else pipe.launches()
            print(name, repr(d), n)
            assert (got == exp).all(), (name, got, exp)
            assert d == text, (name, d)
            assert n == launches, (name, n)
            seen.append(name)
    finally:
        for k, x in _PLAN_KNOBS: ctx.set_tuning(k, x)
    assert seen == list(_PLAN_TEXT)


@pytest.mark.parametrize("dq,nvec", [(13, 200), (60, 96), (65500, 70), (300, 33)])
def test_many_gap_operands(ctx, port, dq, nvec, agg_path):
    """BASELINE configs[4] shape at test scale: combine_or / combine_and_sub / counts pipeline over many GAP
    operands per block column (lane-per-operand run scatter, >= 32 operands) incl. dense GAP (long 1-runs)"""
    nbits = 5 * 65536 + 4000
    words = [port.gen_words(31337, v, dq, nbits) for v in range(nvec)]
    words[3][2048:4096] = 0                                   # NULL block in one operand
    if dq > 60000:
        words[5][0:2048] = 0xFFFFFFFF                         # FULL block
    gv = [bm.bit_import_u32(ctx, w, True) for w in words]
    pv = [port.import_words(w, True, w.size * 32) for w in words]
    assert gv[0].calc_stat()["gap_blocks"] > 0
    agg = bm.aggregator(ctx)
    nwb = 6 * 2048
    o = agg.combine_or(gv)
    assert (o.to_words(nwb) == port.agg_or(pv).to_words(nwb)).all()
    for a, s in [(list(range(nvec)), []), ([0, 1], list(range(2, nvec))), (list(range(0, nvec, 2)), list(range(1, nvec, 2))),
                 ([5], list(range(6, min(nvec, 6 + 40))))]:
        t, _ = agg.combine_and_sub([gv[i] for i in a], [gv[i] for i in s])
        e = port.agg_and_sub([pv[i] for i in a], [pv[i] for i in s])
        assert (t.to_words(nwb) == e.to_words(nwb)).all(), (len(a), len(s))
        pipe = bm.aggregator.pipeline(ctx)
        ag = pipe.add()
        for i in a: ag.add(gv[i], 0)
        for i in s: ag.add(gv[i], 1)
        pipe.complete()
        assert int(agg.combine_and_sub(pipe)[0]) == e.count()
        ctx.set_tuning("pipe_staged", 1)               # GAP planes expanded into LDS by the staged kernel
        try:                                           # (plane tables are built at complete() when the knob forces them)
            pipe2 = bm.aggregator.pipeline(ctx)
            ag2 = pipe2.add()
            for i in a: ag2.add(gv[i], 0)
            for i in s: ag2.add(gv[i], 1)
            pipe2.complete()
            assert int(agg.combine_and_sub(pipe2)[0]) == e.count()
        finally:
            ctx.set_tuning("pipe_staged", -1)


@pytest.mark.parametrize("nvec,ncols", [(24, 1), (64, 16), (257, 7), (1024, 3)])
def test_small_collection_direct_path(ctx, port, nvec, ncols):
    """combine_and_sub over a small collection (few block columns, >= 24 operands) is ONE launch straight from the
    descriptor tables (k_and_sub_direct): same blocks, kinds and bits as the oracle and as the row-table pipeline
    path (pipe_split 0), over BIT / GAP / FULL / NULL operands, ragged lengths, empty AND groups' columns and
    operand counts up to the kernel's list capacity"""
    rng = np.random.default_rng(nvec * 31 + ncols)
    nbits = ncols * 65536 - 77
    words = []
    for v in range(nvec):
        nb = nbits if v % 6 else max(65536 - 77, nbits - 2 * 65536)          # ragged
        kind = v % 4
        w = port.gen_words(99, v, 64000 if kind < 2 else 600, nb)             # dense BIT / sparse GAP
        w |= port.gen_words(99, 0xFFFFFFFF, 3000, nb)                         # shared component (the AND survives)
        nw = (nb + 31) // 32
        if nb % 32: w[nw - 1] &= (1 << (nb % 32)) - 1
        w[nw:] = 0
        for b in range(w.size // 2048):
            r = rng.integers(0, 40)
            if r == 0 and v % 9 == 8: w[b * 2048:(b + 1) * 2048] = 0
            elif r < 6 and (b + 1) * 65536 <= nb: w[b * 2048:(b + 1) * 2048] = 0xFFFFFFFF
        words.append(w)
    gv = [bm.bit_import_u32(ctx, w, True) for w in words]
    pv = [port.import_words(w, True, w.size * 32) for w in words]
    nwb = ncols * 2048
    agg = bm.aggregator(ctx)
    na = nvec - nvec // 8
    cases = [(list(range(nvec)), []), (list(range(na)), list(range(na, nvec))), ([1], list(range(2, nvec))),
             ([i for i in range(nvec) if i % 6], [])]
    try:
        for a, s in cases:
            e = port.agg_and_sub([pv[i] for i in a], [pv[i] for i in s])
            for split in (-1, 0):
                ctx.set_tuning("pipe_split", split)
                t, any_ = agg.combine_and_sub([gv[i] for i in a], [gv[i] for i in s])
                assert (t.to_words(nwb) == e.to_words(nwb)).all(), (len(a), len(s), split)
                assert t.block_table()[0].tolist() == (e.flatten()[0].tolist() + [0] * ncols)[:t.info()["nblocks"]]
                assert any_ == (e.count() != 0) and t.count() == e.count()
                # find_first_and_sub: whole vector, a multi-block hint, a one-block hint (bit mask)
                bits = np.flatnonzero(np.unpackbits(e.to_words(nwb).view(np.uint8), bitorder="little"))
                assert agg.find_first_and_sub([gv[i] for i in a], [gv[i] for i in s]) == ((True, int(bits[0])) if bits.size else (False, 0))
                hints = [(100, 60000)] + ([(65536 + 9, min(nbits - 1, 3 * 65536 + 5))] if ncols > 2 else [])
                if bits.size: hints.append((int(bits[bits.size // 2]), int(bits[bits.size // 2]) | 0xFFFF))
                for frm, to in hints:
                    one = agg.set_range_hint(frm, to)
                    cand = bits[(bits >= frm) & (bits <= to)] if one else bits[(bits >= (frm >> 16) << 16) & (bits < ((to >> 16) + 1) << 16)]
                    f, idx = agg.find_first_and_sub([gv[i] for i in a], [gv[i] for i in s])
                    assert f == (cand.size > 0) and (not f or idx == cand[0]), (frm, to, split)
                agg.reset_range_hint()
        # combine_or: with and without result optimisation (block kinds follow opt_mode, src/bmaggregator.h:1658)
        for sel in (list(range(nvec)), [i for i in range(nvec) if i % 4 >= 2], [i for i in range(nvec) if i % 4 >= 2 and i % 9 != 8][:30]):
            if len(sel) < 24: continue
            for opt in (False, True):
                eo = port.agg_or([pv[i] for i in sel], opt)
                for split in (-1, 0):
                    ctx.set_tuning("pipe_split", split)
                    agg.set_optimization(opt)
                    o = agg.combine_or([gv[i] for i in sel])
                    assert (o.to_words(nwb) == eo.to_words(nwb)).all(), (len(sel), split)
                    assert o.block_table()[0].tolist() == (eo.flatten()[0].tolist() + [0] * ncols)[:o.info()["nblocks"]], (len(sel), split, opt)
            agg.set_optimization(False)
    finally:
        ctx.set_tuning("pipe_split", -1)
        agg.reset_range_hint()


@pytest.mark.parametrize("nops", [3, 30])
def test_find_first_launch_windows(ctx, port, nops, agg_path):
    """find_first_and_sub visits the block columns in ascending launch windows that grow fourfold (every wave looks at
    the best hit so far and leaves when its column lies behind it): the answer never depends on the window size
    (ff_window knob: -1 = one launch, N = first window of N columns), on where the first hit lies, or on the kernel
    (wave-per-column for short operand lists, k_direct for long ones); with and without a range hint"""
    ncols = 45
    nbits = ncols * 65536 - 1000
    rng = np.random.default_rng(nops)
    agg = bm.aggregator(ctx)
    try:
        for first_col in (0, 1, 6, 7, 22, 44, None):
            # the AND survives only from `first_col` on: a shared component restricted to the columns behind it
            common = port.gen_words(808, 0xFFFFFFFF, 300, nbits)
            if first_col is None: common[:] = 0
            else: common[:first_col * 2048] = 0
            words = []
            for v in range(nops):
                w = port.gen_words(808, v, 2000 if v % 3 else 40000, nbits) | common       # GAP and bit operands
                if v == 1: w[:(ncols if first_col is None else first_col) * 2048] = 0          # nothing survives before first_col
                words.append(w)
            subw = port.gen_words(809, 1, 500, nbits)
            gv = [bm.bit_import_u32(ctx, w, True) for w in words]
            gs = bm.bit_import_u32(ctx, subw, True)
            acc = words[0].copy()
            for w in words[1:]: acc &= w
            acc &= ~subw
            bits = np.flatnonzero(np.unpackbits(acc.view(np.uint8), bitorder="little"))
            for win in (0, -1, 1, 2, 5, 64):
                ctx.set_tuning("ff_window", win)
                f, idx = agg.find_first_and_sub(gv, [gs])
                assert f == (bits.size > 0) and (not f or idx == bits[0]), (first_col, win, f, idx, bits[:1])
                if bits.size > 10:
                    frm, to = int(bits[5]) + 1, nbits - 1                                   # hint starting behind the 6th hit
                    one = agg.set_range_hint(frm, to)                                      # one-block hints are bit-exact
                    cand = bits[bits >= frm] if one else bits[bits >= (frm >> 16) << 16]
                    f, idx = agg.find_first_and_sub(gv, [gs])
                    assert f and idx == cand[0], (first_col, win)
                    agg.reset_range_hint()
    finally:
        ctx.set_tuning("ff_window", 0)
        agg.reset_range_hint()


@pytest.mark.parametrize("dq,nvec,nsub", [(200, 40, 0), (60, 300, 0), (300, 64, 9), (350, 33, 3), (13, 257, 2), (65500, 36, 1)])
def test_gap_only_pipeline_counting_formulation(ctx, port, dq, nvec, nsub):
    """counts pipelines whose operands hold no bit-block take the counting formulation (k_pipe_counts_gapcount: byte
    counters of 1-run starts / ends per position + one prefix scan, cover == n): same counts as the run-by-run kernel
    (gap_count 0) and the oracle; more than 255 operands (two counting chunks), SUB groups, FULL / NULL blocks, dense GAP
    (long 1-runs), several groups in one pipeline, block-range runs"""
    nblk = 5
    nbits = nblk * 65536 - 333
    rng = np.random.default_rng(dq + nvec)
    common = port.gen_words(5150, 0xFFFFFFFF, max(dq // 2, 3), nbits)
    words = []
    for v in range(nvec + nsub):
        w = port.gen_words(5150, v, dq, nbits)
        if v < nvec: w |= common                                        # the AND survives
        if v % 11 == 5: w[2048:4096] = 0xFFFFFFFF                       # FULL block
        if v % 13 == 7 and v >= nvec: w[3 * 2048:4 * 2048] = 0          # NULL block in a SUB operand
        words.append(w)
    gv = [bm.bit_import_u32(ctx, w, True) for w in words]
    pv = [port.import_words(w, True, nbits) for w in words]
    assert all(v.calc_stat()["bit_blocks"] == 0 for v in gv), "the case must stay GAP-only"
    groups = [(list(range(nvec)), list(range(nvec, nvec + nsub))), (list(range(0, nvec, 2)), []), (list(range(nvec // 2)), list(range(nvec, nvec + nsub))[:1])]
    exp = port.pipeline_counts([([pv[i] for i in a], [pv[i] for i in s]) for a, s in groups])
    pipe = bm.aggregator.pipeline(ctx)
    for a, s in groups:
        ag = pipe.add()
        for i in a: ag.add(gv[i], 0)
        for i in s: ag.add(gv[i], 1)
    pipe.complete()
    agg = bm.aggregator(ctx)
    try:
        ctx.set_tuning("pipe_split", 0)                  # (few items with long lists would take the workgroup-split kernel)
        ctx.set_tuning("and_rows", 0)                    # (round 5: GAP-only pipelines default to k_agg_and_rows, test_and_rows_kernel)
        for gc in (1, 0, -1):
            ctx.set_tuning("gap_count", gc)
            if gc == 1: assert "gapcount" in pipe.describe()
            if gc == 0: assert "gapcount" not in pipe.describe()
            got = agg.combine_and_sub(pipe)
            assert (got == exp).all(), (gc, got, exp)
            parts = sum(agg._run_pipeline(pipe, a, b).astype(np.int64) for a, b in [(0, 2), (2, 3), (3, nblk)])
            assert (parts == exp.astype(np.int64)).all(), gc
        # the materialising form (combine_and_sub over GAP-only operands stores the column bitmap as a result block):
        # same bits and block kinds as the run-by-run kernel and the oracle
        ctx.set_tuning("direct_cols", 0)                 # (so few columns would take the one-launch kernel)
        for a, s in groups[:2]:
            e = port.agg_and_sub([pv[i] for i in a], [pv[i] for i in s])
            for gc in (1, 0):
                ctx.set_tuning("gap_count", gc)
                t, any_ = agg.combine_and_sub([gv[i] for i in a], [gv[i] for i in s])
                assert (t.to_words(nblk * 2048) == e.to_words(nblk * 2048)).all(), (gc, len(a), len(s))
                assert t.block_table()[0].tolist() == (e.flatten()[0].tolist() + [0] * nblk)[:t.info()["nblocks"]] and any_ == (e.count() != 0)
        ctx.set_tuning("direct_cols", 384)
        ctx.set_tuning("pipe_split", -1); ctx.set_tuning("gap_count", -1); ctx.set_tuning("and_rows", -1)
        assert (agg.combine_and_sub(pipe) == exp).all()   # default selection (workgroup-split kernel for so few items)
    finally:
        ctx.set_tuning("gap_count", -1); ctx.set_tuning("pipe_split", -1); ctx.set_tuning("direct_cols", 384); ctx.set_tuning("and_rows", -1)


@pytest.mark.parametrize("common_bits,own_dq,nvec", [(1, 30, 40), (40, 100, 70), (400, 100, 90), (520, 40, 36),
                                                     (700, 200, 50)])
def test_sparse_state_of_gap_lists(ctx, port, common_bits, own_dq, nvec, agg_path):
    """AND / SUB lists of GAP operands whose intersection SURVIVES (a shared component): the accumulator turns
    into a candidate list (<= 1024 bits) after the first operands and every further operand is a membership
    test (bmx_device.h gap_apply_sparse) -- entry at list start, after the wave-mode head, after a lane-mode
    step; compaction as candidates die; GAP blocks longer than 1024 runs; block rebuilt for combine_and_sub."""
    nblk = 4
    nbits = nblk * 65536
    rng = np.random.default_rng(common_bits * 7 + nvec)
    common = np.zeros(nbits // 32, np.uint32)
    for b in range(nblk):                                              # block 3 gets no shared bits (dies)
        if b == 3: continue
        pos = rng.choice(65536, size=common_bits, replace=False) + b * 65536
        np.bitwise_or.at(common, pos >> 5, (np.uint32(1) << (pos & 31).astype(np.uint32)))
    words = []
    for v in range(nvec):
        w = port.gen_words(4242, v, own_dq, nbits) | common
        if v % 7 == 3:                                                 # a long GAP block (~1100 runs) among them
            extra = rng.choice(65536, size=450, replace=False) + 65536
            np.bitwise_or.at(w, extra >> 5, (np.uint32(1) << (extra & 31).astype(np.uint32)))
        words.append(w)
    subs = [port.gen_words(999, 100 + v, 2000, nbits) for v in range(nvec // 2)]   # ~3 %: each kills few candidates
    gv = [bm.bit_import_u32(ctx, w, True) for w in words]
    pv = [port.import_words(w, True, nbits) for w in words]
    gs = [bm.bit_import_u32(ctx, w, True) for w in subs]
    ps = [port.import_words(w, True, nbits) for w in subs]
    if common_bits + own_dq < 600:                                     # (the last case mixes BIT and GAP blocks)
        assert gv[0].calc_stat()["gap_blocks"] >= 3
    agg = bm.aggregator(ctx)
    nwb = nblk * 2048
    for na, ns in [(nvec, 0), (nvec, len(subs)), (3, len(subs)), (nvec // 2, 1), (2, 2), (34, 0)]:
        a, s = gv[:na], gs[:ns]
        e = port.agg_and_sub(pv[:na], ps[:ns])
        t, _ = agg.combine_and_sub(a, s)
        assert (t.to_words(nwb) == e.to_words(nwb)).all(), (na, ns)
        pipe = bm.aggregator.pipeline(ctx)
        ag = pipe.add()
        for x in a: ag.add(x, 0)
        for x in s: ag.add(x, 1)
        pipe.complete()
        assert int(agg.combine_and_sub(pipe)[0]) == e.count(), (na, ns)
        found, pos = agg.find_first_and_sub(a, s)
        ef, epos = port.find_first_and_sub(pv[:na], ps[:ns])
        assert found == ef and (not found or pos == epos)


def test_shift_right_and(ctx, port):
    """aggregator::combine_shift_right_and (src/bmaggregator.h:2494): the reference's own known answers
    (tests/stress/t.cpp:10640-10800, table in test_oracle_golden.shift_right_and_kats) and seeded dense /
    mixed operands vs the oracle -- pattern lengths 2..33 (register path, carries across block borders),
    40 and 100 operands (shifts across words through the LDS window), GAP / FULL / NULL neighbours."""
    from test_oracle_golden import shift_right_and_kats
    agg = bm.aggregator(ctx)
    for a, b, exp in shift_right_and_kats():
        gv, pv = [], []
        for spec in (a, b):
            nbits = 0xFFFFFFFF if spec.get("range", (0, 0))[1] > (1 << 30) else 5 * 65536
            v = port.new(nbits)
            for i in spec.get("bits", []): v.set_bit(i)
            if "range" in spec: v.set_range(*spec["range"])
            v.optimize()
            pv.append(v)
            gv.append(bm.bvector.from_block_table(ctx, nbits, *v.flatten()))
        agg.set_optimization(True)
        t, f = agg.combine_shift_right_and(gv)
        e, ef = port.agg_shift_right_and(pv, True, False)
        assert t.count() == exp["count"] == e.count() and f == ef == (exp["count"] > 0)
        k = t.block_table()[0].tolist()
        assert k == e.flatten()[0].tolist()
        if "blocks" in exp:
            assert k.count(bm.BIT) + k.count(bm.GAP) == exp["blocks"]
        nw = min(t.info()["nblocks"], 8) * 2048
        assert (t.to_words(nw) == e.to_words(nw)).all()
        agg.set_optimization(False)
    nbits = 6 * 65536 + 1234
    nw = 7 * 2048
    rng = np.random.default_rng(2024)
    for dq, n in [(64000, 2), (64000, 9), (65300, 33), (65400, 40), (65500, 100), (60000, 5), (32768, 3), (655, 2)]:
        ws = []
        for v in range(min(n, 12)):
            w = port.gen_words(777 + dq, v, dq, nbits)
            r = int(rng.integers(0, 6))
            if r == 0: w[2048 * 2:2048 * 3] = 0xFFFFFFFF                 # FULL block (and a FULL lower neighbour)
            if r == 1: w[2048 * 4:2048 * 5] = 0                          # NULL block
            if r == 2: w[2048:2048 * 2] = 0xFFFFFFFF; w[2048 + 5] = 0x7FFFFFFF   # dense GAP block
            ws.append(w)
        sel = [i % len(ws) for i in range(n)]
        gv = [bm.bit_import_u32(ctx, w, True) for w in ws]
        pv = [port.import_words(w, True, nbits) for w in ws]
        for opt in (False, True):
            agg.set_optimization(opt)
            t, f = agg.combine_shift_right_and([gv[i] for i in sel])
            e, ef = port.agg_shift_right_and([pv[i] for i in sel], opt, False)
            assert f == ef and (t.to_words(nw) == e.to_words(nw)).all(), (dq, n, opt)
            assert t.block_table()[0].tolist() == e.flatten()[0].tolist()
        agg.set_optimization(False)
        ta, fa = agg.combine_shift_right_and([gv[i] for i in sel], any=True)
        ea, efa = port.agg_shift_right_and([pv[i] for i in sel], False, True)
        assert fa == efa and (ta.to_words(nw) == ea.to_words(nw)).all()
        agg.set_compute_count(True)
        agg.combine_shift_right_and([gv[i] for i in sel])
        assert agg.count() == port.agg_shift_right_and_count([pv[i] for i in sel])
        agg.set_compute_count(False)
    # more operands than bits in a block: the window of src[0] starts one whole block (and 463 bits) lower
    pl = port.new(3 * 65536)
    pl.set_range(5, 3 * 65536 - 1)
    pl.optimize()
    gl = bm.bvector.from_block_table(ctx, 3 * 65536, *pl.flatten())
    n_long = 66000
    t, f = agg.combine_shift_right_and([gl] * n_long)
    e, ef = port.agg_shift_right_and([pl] * n_long, False, False)
    assert f == ef and t.count() == e.count() == 3 * 65536 - 5 - (n_long - 1)
    assert (t.to_words(3 * 2048) == e.to_words(3 * 2048)).all()
    # member form: add() + combine_shift_right_and(); empty list => cleared target (:2499)
    t, f = agg.combine_shift_right_and([])
    assert not f and t.count() == 0


def test_bm64_vectors(ctx, port, golden):
    """vectors above 2^32 bits (bit positions are 64-bit through the whole ABI; 99,183 blocks) vs the fixtures the
    reference generated in its BM64ADDR build: pairwise ops, aggregator, shift-right-and, pipeline, rank / select
    with positions beyond 2^32"""
    g = golden["bm64"]
    ksha = lambda v: sha(np.asarray(v.block_table()[0], np.uint8))
    pv = [bm64_build(port, s_) for s_ in range(BM64_NVEC)]
    from cases import BM64_NBITS
    vecs = [bm.bvector.from_block_table(ctx, BM64_NBITS, *p.flatten()) for p in pv]
    assert [v.count() for v in vecs] == g["count"]
    ops = [bm.bvector.bit_and, bm.bvector.bit_or, bm.bvector.bit_xor, bm.bvector.bit_sub]
    cnts = [bm.count_and, bm.count_or, bm.count_xor, bm.count_sub]
    for op in range(4):
        e = g["op2"][str(op)]
        t = ops[op](vecs[0], vecs[1], bm.opt_compress)
        kk, ek = t.block_table()[0], port.op2(op, pv[0], pv[1], True).flatten()[0]
        assert t.count() == e["count"] == cnts[op](vecs[0], vecs[1])
        assert kk.tolist() == ek.tolist()
    agg = bm.aggregator(ctx)
    t, any_ = agg.combine_and_sub(vecs[:3], vecs[3:])
    assert t.count() == g["agg_and_sub"]["count"] and ksha(t) == g["agg_and_sub"]["kinds_sha"] and any_
    f, idx = agg.find_first_and_sub(vecs[:3], vecs[3:])
    assert [f, idx] == [bool(g["agg_and_sub"]["find_first"][0]), g["agg_and_sub"]["find_first"][1]]
    assert agg.combine_or(vecs).count() == g["agg_or"]["count"]
    agg.set_optimization(True)
    t, f = agg.combine_shift_right_and(vecs[:3])
    assert t.count() == g["shift_right_and"]["count"] and f == g["shift_right_and"]["found"] and ksha(t) == g["shift_right_and"]["kinds_sha"]
    pipe = bm.aggregator.pipeline(ctx)
    for a, s_ in [(vecs[:2], []), (vecs[:3], vecs[3:]), (vecs[1:], [])]:
        ag = pipe.add()
        for x in a: ag.add(x, 0)
        for x in s_: ag.add(x, 1)
    pipe.complete()
    assert [int(x) for x in agg.combine_and_sub(pipe)] == g["pipeline_counts"]
    rs = vecs[0].build_rs_index()
    rq, sq = bm64_queries(g["count"][0])
    assert rs.count() == g["rs"]["count"] and [int(x) for x in vecs[0].rank(rq, rs)] == g["rs"]["rank"]
    found, pos = vecs[0].select(sq, rs)
    assert found.astype(int).tolist() == g["rs"]["select_found"]
    assert [int(p_) if f_ else 0 for p_, f_ in zip(pos, found)] == g["rs"]["select_pos"]


def test_full_size_rank_select(ctx, port):
    """BASELINE configs[3]: rs-index + rank / select on a 4e9-bit vector (10 % and the mixed 1 % case).
    Size-independent properties: rank(select(r)) == r and select(rank(n)) <= n with bit(n) deciding equality,
    rank(N-1) == count, rank is monotone with unit steps, count_range additivity; sampled blocks vs the oracle
    on identically generated words."""
    nbits = 4_000_000_000
    rng = np.random.default_rng(99)
    for dq in (6554, 655):
        v = bm.bvector.generate(ctx, SEED, 42, dq, nbits)
        rs = v.build_rs_index()
        cnt = v.count()
        assert rs.count() == cnt and v.rank(np.array([nbits - 1], np.uint64), rs)[0] == cnt
        r = rng.integers(1, cnt + 1, size=200_000).astype(np.uint64)
        found, pos = v.select(r, rs)
        assert found.all() and (v.rank(pos, rs) == r).all()
        assert (v.rank(pos - np.uint64(1), rs)[pos > 0] == (r - np.uint64(1))[pos > 0]).all()     # pos is a set bit
        f2, _ = v.select(np.array([0, cnt + 1], np.uint64), rs)
        assert not f2.any()
        n = np.sort(rng.integers(0, nbits, size=200_000).astype(np.uint64))
        rk = v.rank(n, rs)
        assert (np.diff(rk.astype(np.int64)) >= 0).all() and (np.diff(rk.astype(np.int64)) <= np.diff(n.astype(np.int64))).all()
        mid = (n[:-1] + n[1:]) // np.uint64(2)
        cr = v.count_range(n[:-1], n[1:], rs)
        left = v.count_range(n[:-1], mid, rs); right = v.count_range(mid + np.uint64(1), n[1:], rs)
        ok = mid < n[1:]
        assert (cr[ok] == (left + right)[ok]).all()
        for nb0 in (0, 30517, 61035):                     # rank inside sampled blocks vs popcounts of the oracle's words
            nw = min(2048, (nbits + 31) // 32 - nb0 * 2048)
            w = port.gen_words(SEED, 42, dq, nbits, word_off=nb0 * 2048, nwords=nw)
            bits = np.unpackbits(w.view(np.uint8), bitorder="little")
            q = np.sort(rng.integers(0, nw * 32, size=300)).astype(np.uint64)
            base = v.rank(np.array([nb0 * 65536 - 1], np.uint64), rs)[0] if nb0 else np.uint64(0)
            got = v.rank(q + np.uint64(nb0 * 65536), rs) - base
            assert (got == np.cumsum(bits)[q.astype(np.int64)]).all()
        del rs, v


def test_full_size_or_of_4096_sparse_vectors(ctx, port):
    """BASELINE configs[4]: combine_or over 4096 sparse 4e9-bit vectors (0.02 %, every block GAP; the column-tile
    kernel).  Properties: OR(all) == OR(OR(first half), OR(second half)); |OR| <= sum of counts; sampled block
    columns equal the OR of the oracle's identically generated words."""
    nbits, nvec, dq = 4_000_000_000, 4096, 13
    vecs = [bm.bvector.generate(ctx, SEED, 10000 + i, dq, nbits) for i in range(nvec)]
    assert vecs[0].calc_stat()["bit_blocks"] == 0
    agg = bm.aggregator(ctx)
    t = agg.combine_or(vecs)
    tc = t.count()
    h1, h2 = agg.combine_or(vecs[:2048]), agg.combine_or(vecs[2048:])
    t2 = agg.combine_or([h1, h2])
    assert t2.count() == tc and bm.count_xor(t, t2) == 0
    assert bm.count_and(t, h1) == h1.count() and tc <= sum(v.count() for v in vecs[::512]) * 512 * 1.2
    p = 1.0 - (1.0 - dq / 65536) ** nvec
    assert abs(tc - p * nbits) < 1e-3 * nbits
    for nb0 in (5, 61035):
        nw = min(2048, (nbits + 31) // 32 - nb0 * 2048)
        acc = np.zeros(nw, np.uint32)
        for i in range(nvec):
            acc |= port.gen_words(SEED, 10000 + i, dq, nbits, word_off=nb0 * 2048, nwords=nw)
        got = t.to_words((nb0 + 1) * 2048)[nb0 * 2048: nb0 * 2048 + nw]
        assert (got == acc).all()
    # the three ways the library has of doing this aggregation at FULL size give the same vector bit for bit and block kind
    # for block kind: the row kernel (tile directories, the default first call), the column-tile kernel (or_rows 0) and the
    # streaming kernel over the prepared packed collection
    kinds = t.block_table()[0]
    ctx.set_tuning("or_rows", 0)
    try:
        t_tiled = agg.combine_or(vecs)
    finally:
        ctx.set_tuning("or_rows", -1)
    assert t_tiled.count() == tc and bm.count_xor(t, t_tiled) == 0 and (t_tiled.block_table()[0] == kinds).all()
    assert ctx.pack_stats()["collections"] == 0
    ctx.collection_prepare(vecs, bm.ROLE_OR)
    assert ctx.pack_stats()["collections"] == 1
    t_packed = agg.combine_or(vecs)
    assert t_packed.count() == tc and bm.count_xor(t, t_packed) == 0 and (t_packed.block_table()[0] == kinds).all()
    t_shuffled = agg.combine_or(vecs[::-1])                          # any order: still the whole collection
    assert bm.count_xor(t, t_shuffled) == 0
    for nb0 in (5, 61035):
        nw = min(2048, (nbits + 31) // 32 - nb0 * 2048)
        a0 = t.to_words((nb0 + 1) * 2048)[nb0 * 2048: nb0 * 2048 + nw]
        assert (t_packed.to_words((nb0 + 1) * 2048)[nb0 * 2048: nb0 * 2048 + nw] == a0).all()
    del t_tiled, t_packed, t_shuffled


def test_slice_scanner_vs_numpy(ctx):
    """bit-sliced equality search (the sparse_vector_scanner call pattern) against a plain numpy
    column: counts of a batch, result vectors, first positions; a value with a bit above every plane and a
    value whose plane is absent must find nothing (src/bmsparsevec_algo.h:2621)"""
    rng = np.random.default_rng(8)
    n = 3 * 65536 + 999
    col = rng.integers(0, 200, size=n).astype(np.uint32)
    col[::5000] = 3000 + (np.arange(0, n, 5000) % 5).astype(np.uint32)          # rare wide values
    nplanes = 12
    slices = []
    for b in range(nplanes):
        bits = ((col >> b) & 1).astype(np.uint8)
        if not bits.any():
            slices.append(None); continue
        w = np.packbits(np.concatenate([bits, np.zeros((-n) % 32, np.uint8)]), bitorder="little").view(np.uint32)
        slices.append(bm.bit_import_u32(ctx, w, True))
    assert any(s is None for s in slices)
    sc = bm.slice_scanner(ctx, slices, size=n)
    vals = [1, 7, 100, 199, 200, 255, 3000, 3004, 3005, 4095, 1 << 11, 1 << 20]
    cnt = sc.find_eq_counts(vals)
    assert cnt.tolist() == [int((col == v).sum()) for v in vals]
    for v in vals:
        t, found = sc.find_eq(v)
        idx = np.flatnonzero(col == v)
        assert found == (idx.size > 0)
        if found:
            got = np.flatnonzero(np.unpackbits(t.to_words((n + 31) // 32).view(np.uint8), bitorder="little")[:n])
            assert (got == idx).all()
        f, pos = sc.find_first_eq(v)
        assert f == (idx.size > 0) and (not f or pos == idx[0])
    t0, f0 = sc.find_eq(0)                                   # value 0 = find_zero (src/bmsparsevec_algo.h:4366)
    assert f0 == bool((col == 0).any()) and t0.count() == int((col == 0).sum())
    assert sc.find_eq_counts([0, 7, 0]).tolist() == [int((col == 0).sum()), int((col == 7).sum()), int((col == 0).sum())]


@pytest.mark.parametrize("case", ["dense12", "wide32", "gap_planes"])
def test_batched_equality_counts_by_transposition(ctx, case):
    """find_eq_counts in one pass over the planes (bmx_slice_eq_counts: bit-matrix transposition + hash lookup) against
    the reference's formulation (one AND-SUB group per query, pipeline) and numpy: duplicates, value 0 with NULL
    elements, values with a bit above every plane / in an absent plane, rows past size(), planes of every block kind
    (GAP planes are expanded first), more unique values than one launch takes (2048)"""
    rng = np.random.default_rng({"dense12": 31, "wide32": 32, "gap_planes": 33}[case])
    n = 6 * 65536 + 1234
    if case == "dense12":
        col = rng.integers(0, 4000, size=n).astype(np.uint64); nplanes = 12
    elif case == "wide32":
        col = np.where(rng.random(n) < 0.3, rng.integers(1, 1 << 32, size=n), rng.integers(0, 50, size=n)).astype(np.uint64); nplanes = 32
    else:   # long runs of equal values: GAP / FULL / NULL plane blocks
        col = np.repeat(rng.integers(0, 64, size=n // 499 + 1), 499)[:n].astype(np.uint64); nplanes = 7
        col[65536:2 * 65536] = 63                                      # FULL blocks in the low planes
    col &= ~np.uint64(1 << 5)                                           # plane 5 is absent
    notnull = rng.random(n) < 0.9
    col[~notnull] = 0
    def upload(bits):
        w = np.packbits(np.concatenate([bits.astype(np.uint8), np.zeros((-n) % 32, np.uint8)]), bitorder="little").view(np.uint32)
        return bm.bit_import_u32(ctx, w, True)
    slices = []
    for b in range(nplanes):
        bits = ((col >> np.uint64(b)) & np.uint64(1)).astype(bool)
        slices.append(upload(bits) if bits.any() else None)
    assert slices[5] is None
    if case == "gap_planes":
        assert any(s is not None and s.calc_stat()["gap_blocks"] for s in slices)
    nn = upload(notnull)
    present = [int(x) for x in rng.choice(col[col > 0], 40)]
    vals = present + [0, 1, 2, 32, 33, (1 << nplanes) - 1, 1 << nplanes, (1 << 40) + 3, present[0], 0, present[1]]
    for size, with_null in ((n, False), (n, True), (n - 70000, True), (65536, False)):
        sc = bm.slice_scanner(ctx, slices, size=size, not_null=nn if with_null else None)
        valid = (notnull if with_null else np.ones(n, bool))[:size]
        c = col[:size]
        exp = [int(((c == np.uint64(v)) & (valid if v == 0 else True)).sum()) if v < (1 << 63) else 0 for v in vals]
        got_t = sc.find_eq_counts(vals, method="transpose")
        assert got_t.tolist() == exp, (case, size, with_null)
        if size == n:            # (the group formulation has no notion of size(): a real container holds no bits past it)
            assert sc.find_eq_counts(vals, method="pipeline").tolist() == exp, (case, with_null)
    # more unique values than one launch takes: every distinct value of the column + misses
    sc = bm.slice_scanner(ctx, slices, size=n)
    uniq, cnts = np.unique(col, return_counts=True)
    many = [int(v) for v in uniq[uniq > 0]][:5000] + [int(x) for x in rng.integers(1, 1 << min(nplanes, 31), size=3000)]
    lut = {int(v): int(k) for v, k in zip(uniq, cnts)}
    got = sc.find_eq_counts(many)
    assert got.tolist() == [lut.get(v, 0) for v in many]
    # the two table forms (k_slice_eq_counts: 2,048 values per pass; k_slice_eq_counts_big: 9,216) on small and large
    # batches, incl. more values than ONE pass of the big form takes
    more = many + [int(x) for x in rng.integers(1, 1 << min(nplanes, 31), size=14000)]
    exp_small = [lut.get(v, 0) if v else int((col == 0).sum()) for v in vals]
    try:
        for eb, shape in ((0, 1), (1, 0), (1, 1), (1, 2), (-1, 1), (-1, 2)):
            ctx.set_tuning("eq_big", eb); ctx.set_tuning("eq_big_shape", shape)
            assert sc.find_eq_counts(vals).tolist() == exp_small, (eb, shape)
            assert sc.find_eq_counts(more).tolist() == [lut.get(v, 0) for v in more], (eb, shape)
    finally:
        ctx.set_tuning("eq_big", -1); ctx.set_tuning("eq_big_shape", 2)


def test_packed_collection_kernel_shapes(port):
    """every launch shape of k_coll_apply (256 / 512 threads, with and without the second batch in flight, a wave's batch as
    four 1-KiB pieces or one 4-KiB piece) and both bag formats (split: single-bit runs as 16-bit positions behind the
    multi-bit runs; plain: every run a 32-bit interval) must produce the oracle's bits and block kinds for OR, AND-SUB
    (the SUB bag is a polarity-1 bag too) and the counts; the operands mix isolated bits, wide runs, NULL / FULL blocks"""
    rng = np.random.default_rng(77)
    nvec, nbits = 96, 5 * 65536 + 4321
    words = _sparse_collection(port, rng, nvec, nbits, 300, long_runs=True, ragged=True)
    pv = [port.import_words(w, True, w.size * 32) for w in words]
    nwb = 6 * 2048
    e_or = port.agg_or(pv, False)
    e_as = port.agg_and_sub(pv[:80], pv[80:])
    for shape, split in [(sh, 1) for sh in range(6)] + [(4, 0), (0, 0)]:      # split: single-bit runs kept as 16-bit positions (default) or not
        c = bm.context(0)
        c.set_tuning("gap_pack", 1); c.set_tuning("coll_shape", shape); c.set_tuning("coll_split", split)
        c.set_tuning("direct_cols", 0); c.set_tuning("pipe_split", 0)
        gv = [bm.bit_import_u32(c, w, True) for w in words]
        agg = bm.aggregator(c)
        o = agg.combine_or(gv)
        assert (o.to_words(nwb) == e_or.to_words(nwb)).all(), shape
        assert o.block_table()[0].tolist() == (e_or.flatten()[0].tolist() + [0] * 8)[:o.info()["nblocks"]], shape
        t, any_ = agg.combine_and_sub(gv[:80], gv[80:])
        assert (t.to_words(nwb) == e_as.to_words(nwb)).all(), shape
        assert t.block_table()[0].tolist() == (e_as.flatten()[0].tolist() + [0] * 8)[:t.info()["nblocks"]], shape
        pipe = bm.aggregator.pipeline(c)
        ag = pipe.add()
        for v in gv[:80]: ag.add(v, 0)
        for v in gv[80:]: ag.add(v, 1)
        pipe.complete()
        assert int(agg.combine_and_sub(pipe)[0]) == e_as.count(), shape
        assert c.pack_stats()["collections"] > 0
        del o, t, pipe, ag, agg, gv
        c.close()


def _bits_of(t, n):
    return np.unpackbits(t.to_words((n + 31) // 32).view(np.uint8), bitorder="little")[:n].astype(bool)


@pytest.mark.parametrize("case", ["dense12", "sparse40", "gap_planes"])
def test_slice_scanner_range_search_vs_numpy(ctx, case):
    """find_gt / find_ge / find_lt / find_le / find_range / find_zero / find_nonzero (src/bmsparsevec_algo.h:
    1135-1174, 2290, 2690-2880, 4464) against a plain numpy column, incl. NULL elements (stored as 0, excluded
    wherever the predicate admits 0: needs_null_correct_*, :1703-1735), absent planes, bounds with bits above
    every plane, rows past size() and planes of every block kind"""
    rng = np.random.default_rng({"dense12": 21, "sparse40": 22, "gap_planes": 23}[case])
    n = 5 * 65536 + 4321
    if case == "dense12":
        col = rng.integers(0, 4000, size=n).astype(np.uint64); nplanes = 12
    elif case == "sparse40":
        col = np.where(rng.random(n) < 0.01, rng.integers(1, 1 << 40, size=n), 0).astype(np.uint64); nplanes = 40
    else:   # long runs of equal values: GAP / FULL / NULL plane blocks
        col = np.repeat(rng.integers(0, 64, size=n // 997 + 1), 997)[:n].astype(np.uint64); nplanes = 7
        col[65536:2 * 65536] = 63                                      # FULL blocks in the low planes
    notnull = rng.random(n) < 0.9
    col[~notnull] = 0
    def upload(bits):
        w = np.packbits(np.concatenate([bits.astype(np.uint8), np.zeros((-n) % 32, np.uint8)]), bitorder="little").view(np.uint32)
        return bm.bit_import_u32(ctx, w, True)
    slices = []
    for b in range(nplanes):
        bits = ((col >> np.uint64(b)) & np.uint64(1)).astype(bool)
        slices.append(upload(bits) if bits.any() else None)
    nn = upload(notnull)
    for with_null in (False, True):
        sc = bm.slice_scanner(ctx, slices, size=n, not_null=nn if with_null else None)
        valid = notnull if with_null else np.ones(n, bool)
        bounds = [0, 1, 2, 5, 63, 64, 100, 1000, 3999, 4000, 4095, 4096, (1 << nplanes) - 1, 1 << nplanes, (1 << 40) + 5]
        bounds += [int(x) for x in rng.choice(col[col > 0], 4)]
        for v in bounds:
            V = np.uint64(v)
            exp = {"gt": col > V, "ge": (col >= V) & (valid if v == 0 else True), "lt": (col < V) & valid, "le": (col <= V) & valid}
            for halves in (1, 0):                      # half-block passes (default) and the whole-block kernel
                ctx.set_tuning("range_halves", halves)
                got = {"gt": sc.find_gt(v), "ge": sc.find_ge(v), "lt": sc.find_lt(v), "le": sc.find_le(v)}
                for k in exp:
                    assert (_bits_of(got[k], n) == exp[k]).all(), (case, with_null, k, v, halves)
                    assert got[k].count() == int(np.count_nonzero(exp[k]))
            ctx.set_tuning("range_halves", 1)
            assert sc.count(bm.CMP_GT, v) == int((col > V).sum())
        for lo, hi in [(0, 0), (0, 10), (5, 5), (10, 3), (100, 3000), (1, (1 << 40)), (4000, 1 << 50)] + \
                      [tuple(int(x) for x in rng.choice(col[col > 0], 2)) for _ in range(3)]:
            a, b = min(lo, hi), max(lo, hi)
            exp = (col >= np.uint64(a)) & (col <= np.uint64(b)) & (valid if a == 0 else True)
            for halves in (1, 0):                      # half-block passes (default) and the four-accumulator kernel
                ctx.set_tuning("range_halves", halves)
                t = sc.find_range(lo, hi)
                assert (_bits_of(t, n) == exp).all(), (case, with_null, lo, hi, halves)
                assert sc.count(bm.CMP_RANGE, lo, hi) == int(exp.sum())
            ctx.set_tuning("range_halves", 1)
        assert (_bits_of(sc.find_zero(), n) == ((col == 0) & valid)).all()
        assert (_bits_of(sc.find_nonzero(), n) == (col != 0)).all()
        t, f = sc.find_eq(0)
        assert (_bits_of(t, n) == ((col == 0) & valid)).all() and f == bool(((col == 0) & valid).any())
    # rows past size() never appear, whatever the planes hold there
    sc = bm.slice_scanner(ctx, slices, size=n - 70000)
    assert sc.find_le(1 << 50).count() == n - 70000 and sc.find_zero().count() == int((col[:n - 70000] == 0).sum())


def test_block_range_shards_add_up(ctx, port):
    """a GPU holds only its block range of every operand.  Shards of the same logical vectors
    (bmx_vec_generate_shard) give partial results whose popcounts add up to the whole-vector result, for the
    OR of sparse GAP vectors (configs[4]) and the AND+COUNT pipeline (configs[2]); shard content equals the
    oracle's words at the shard's offset."""
    nbits, nvec = 40 * 65536 + 12345, 70
    nblocks = 41
    whole = [bm.bvector.generate(ctx, SEED, 300 + i, 40, nbits) for i in range(nvec)]
    agg = bm.aggregator(ctx)
    total_or = agg.combine_or(whole).count()
    dense = [bm.bvector.generate(ctx, SEED, 500 + i, 30000, nbits, with_common=True) for i in range(6)]
    total_and = agg.combine_and_sub(dense[:5], dense[5:])[0].count()
    for world in (1, 2, 3, 8):
        s_or = s_and = 0
        for r in range(world):
            lo, hi = bm.shard_range(nblocks, r, world)
            sh = [bm.bvector.generate(ctx, SEED, 300 + i, 40, nbits, block_range=(lo, hi)) for i in range(nvec)]
            assert sh[0].info()["nblocks"] == hi - lo
            s_or += agg.combine_or(sh).count()
            dsh = [bm.bvector.generate(ctx, SEED, 500 + i, 30000, nbits, with_common=True, block_range=(lo, hi)) for i in range(6)]
            s_and += agg.combine_and_sub(dsh[:5], dsh[5:])[0].count()
            if hi > lo:
                nw = min((hi - lo) * 2048, (nbits + 31) // 32 - lo * 2048)
                w = port.gen_words(SEED, 300, 40, nbits, word_off=lo * 2048, nwords=nw + (nw & 1))[:nw]
                assert (sh[0].to_words(nw) == w).all()
        assert s_or == total_or and s_and == total_and, world


def test_full_size_shift_right_and_properties(ctx, port):
    """combine_shift_right_and on 1e9-bit vectors through size-independent identities: a single operand is a copy;
    shifting against all-ones operands only moves the bits (the count drops by the bits pushed past the end);
    [a, b] equals the AND of b with a moved by one, checked on sampled blocks against the oracle's words."""
    nbits = 1_000_000_000
    a = bm.bvector.generate(ctx, SEED, 77, 20000, nbits)
    b = bm.bvector.generate(ctx, SEED, 78, 40000, nbits)
    ones = bm.bvector.generate(ctx, SEED, 79, 65536, nbits)
    assert ones.count() == nbits
    agg = bm.aggregator(ctx)
    t, f = agg.combine_shift_right_and([a])
    assert f and bm.count_xor(t, a) == 0
    ca = a.count()
    tail = a.to_words((nbits + 31) // 32)[-1]
    for k in (1, 2, 40):
        t, f = agg.combine_shift_right_and([a] + [ones] * k)
        lost = sum((int(tail) >> ((nbits - 1 - j) % 32)) & 1 for j in range(k))       # bits within k of the end
        assert f and t.count() == ca - lost, k
    t, f = agg.combine_shift_right_and([a, b])
    agg.set_compute_count(True)
    agg.combine_shift_right_and([a, b])
    assert agg.count() == t.count()
    agg.set_compute_count(False)
    for nb0 in (0, 9000, 15258):
        nw = min(2048, (nbits + 31) // 32 - nb0 * 2048)
        lo = max(nb0 * 2048 - 2, 0)
        wa = port.gen_words(SEED, 77, 20000, nbits, word_off=lo, nwords=nb0 * 2048 - lo + nw)
        wb = port.gen_words(SEED, 78, 40000, nbits, word_off=nb0 * 2048, nwords=nw)
        bits_a = np.unpackbits(wa.view(np.uint8), bitorder="little")
        off = (nb0 * 2048 - lo) * 32
        shifted = bits_a[off - 1: off - 1 + nw * 32] if off else np.concatenate([[0], bits_a[: nw * 32 - 1]]).astype(np.uint8)
        exp = np.packbits(shifted, bitorder="little").view(np.uint32) & wb
        got = t.to_words((nb0 + 1) * 2048)[nb0 * 2048: nb0 * 2048 + nw]
        assert (got == exp).all(), nb0


def test_range_hint(ctx, port, agg_path):
    """aggregator::set_range_hint (src/bmaggregator.h:481,974): find_first_and_sub visits the block columns of the
    hint only, a one-block hint is also bit-masked (:1470-1512, range_gap_blk_ :980-988); combine_and_sub(pipe)
    honours it when the pipeline options enable search masks (:1312-1346).  Expected values are derived from the
    oracle's materialised result."""
    nbits = 9 * 65536 + 17
    words = [port.gen_words(SEED + 5, v, d, nbits, with_common=True) for v, d in enumerate((20000, 30000, 300, 9000))]
    pv = [port.import_words(w, True, nbits) for w in words]
    gv = [bm.bit_import_u32(ctx, w, True) for w in words]
    e = port.agg_and_sub(pv[:2], pv[2:3])
    bits = np.flatnonzero(np.unpackbits(e.to_words().view(np.uint8), bitorder="little"))
    agg = bm.aggregator(ctx)
    rng = np.random.default_rng(4)
    cases = [(0, nbits - 1), (70000, 70010), (65536 * 3 + 5, 65536 * 3 + 40000), (65536 * 2, 65536 * 5 + 3), (8 * 65536 + 9, nbits - 1),
             (5 * 65536 + 100, 5 * 65536 + 100)]
    cases += [tuple(sorted(int(x) for x in rng.integers(0, nbits, 2))) for _ in range(20)]
    for frm, to in cases:
        one = agg.set_range_hint(frm, to)
        assert one == ((frm >> 16) == (to >> 16))
        f, idx = agg.find_first_and_sub(gv[:2], gv[2:3])
        if one:
            cand = bits[(bits >= frm) & (bits <= to)]
        else:                                      # block-granular: [first bit of block(from), last bit of block(to)]
            cand = bits[(bits >= (frm >> 16) << 16) & (bits < ((to >> 16) + 1) << 16)]
        assert f == (cand.size > 0) and (not f or idx == cand[0]), (frm, to, f, idx, cand[:1])
    agg.reset_range_hint()
    assert agg.find_first_and_sub(gv[:2], gv[2:3]) == (bits.size > 0, int(bits[0]))
    # pipeline with search masks: counts and results restricted to the block columns of the hint
    for opt in (bm.agg_run_options(False, True, True), bm.agg_run_options(True, True, True), bm.agg_run_options(False, True, False)):
        pipe = bm.aggregator.pipeline(ctx, opt)
        for a, s_ in (([0, 1], [2]), ([0, 3], [])):
            ag = pipe.add()
            for i in a: ag.add(gv[i], 0)
            for i in s_: ag.add(gv[i], 1)
        pipe.complete()
        agg.set_range_hint(65536 * 2 + 7, 65536 * 4 + 1)
        agg.combine_and_sub(pipe)
        cnt = pipe.get_bv_count_vector()
        lo, hi = (2, 5) if opt.is_masks() else (0, 10)
        exp = port.pipeline_counts([([pv[0], pv[1]], [pv[2]]), ([pv[0], pv[3]], [])], lo, hi)
        assert (cnt == exp).all(), (opt.is_masks(), cnt, exp)
        if opt.is_make_results():
            for r, c in zip(pipe.get_bv_res_vector(), exp):
                assert (r.count() if r is not None else 0) == c
                k = r.block_table()[0]
                assert not k[:2].any() and not k[5:].any()
        agg.reset_range_hint()


def _rs_mixed_words(rng, nblk=23):
    """-> (nbits, words): nblk blocks of every kind in turn -- NULL, FULL, bit, sparse GAP, GAP of few wide runs, GAP of many short
    runs -- cut 777 bits short of the last block border"""
    nbits = nblk * 65536 - 777
    words = np.zeros(nblk * 2048, np.uint32)
    for nb in range(nblk):
        kind = nb % 6
        if kind == 0: continue                                            # NULL
        lo = nb * 2048
        if kind == 1: words[lo:lo + 2048] = 0xFFFFFFFF                   # FULL
        elif kind == 2: words[lo:lo + 2048] = rng.integers(0, 1 << 32, 2048, dtype=np.uint64).astype(np.uint32)   # bit
        elif kind == 3:                                                   # sparse GAP
            for b in rng.integers(0, 65536, 40): words[lo + (b >> 5)] |= np.uint32(1 << (b & 31))
        elif kind == 4:                                                   # long runs (GAP with few, wide runs)
            words[lo + 100:lo + 900] = 0xFFFFFFFF; words[lo + 1500:lo + 1600] = 0xFFFFFFFF
        else:                                                             # many short runs: still GAP (< 1276 runs)
            for b in rng.integers(0, 65536, 500): words[lo + (b >> 5)] |= np.uint32(1 << (b & 31))
    last_bits = nbits - (nblk - 1) * 65536
    tail = np.unpackbits(words[(nblk - 1) * 2048:].view(np.uint8), bitorder="little"); tail[last_bits:] = 0
    words[(nblk - 1) * 2048:] = np.packbits(tail, bitorder="little").view(np.uint32)
    return nbits, words


def _ones_of(words, nbits):
    """the positions of the set bits, ascending: the NumPy reference of rank and select (read-only: shared between tests)"""
    ones = np.flatnonzero(np.unpackbits(words.view(np.uint8), bitorder="little")[:nbits]).astype(np.uint64)
    ones.setflags(write=False)
    return ones


def _check_rank_np(v, rs, ones, q, what):
    assert (v.rank(q, rs) == np.searchsorted(ones, q, "right").astype(np.uint64)).all(), what


def _check_select_np(v, rs, ones, r, what):
    found, pos = v.select(r, rs)
    live = (r >= 1) & (r <= ones.size)
    exp = np.zeros(r.size, np.uint64)
    exp[live] = ones[(r[live] - np.uint64(1)).astype(np.int64)]
    assert (found == live).all() and (pos == exp).all(), what              # (pos == 0 where not found)


def _check_against_oracle(v, rs, prs, q, r):
    """the same queries against the reference's own rs_index: ties the NumPy rule above to it"""
    assert (v.rank(q, rs) == prs.rank(q)).all()
    found, pos = v.select(r, rs)
    ppos, pfound = prs.select(r)
    assert (found == pfound).all() and (pos[found] == ppos[pfound]).all() and (pos[~found] == 0).all()


_RS_MIXED = []


def _rs_mixed_reference():
    """(nbits, words, ones) of one 23-block vector of every block kind, computed once"""
    if not _RS_MIXED:
        nbits, words = _rs_mixed_words(np.random.default_rng(4242))
        words.setflags(write=False)
        _RS_MIXED.append((nbits, words, _ones_of(words, nbits)))
    return _RS_MIXED[0]


@pytest.mark.parametrize("unroll,lines,sel,selfmt", [(8, 0, 0, 0), (2, 0, 0, 0), (4, 0, 0, 0), (2, 1, 1, 0), (4, 1, 1, 0), (2, 1, 2, 0), (4, 1, 2, 0), (4, 1, (2, 6), 0), (4, 1, (2, 16), 0),
                                                     (4, 1, (2, 0, 1), 0), (2, 1, (2, 6, 1), 0), (4, 1, (2, 16, 1), 0),
                                                     (2, 1, 2, 1), (8, 0, 0, 1), (2, 1, 2, 2), (2, 0, 0, -1)])
def test_rank_select_queries_in_flight_forms(port, unroll, lines, sel, selfmt):
    """k_rank_l<2|4> (fewer lanes per query = more queries in flight), k_rank_lines<2|4> (the vector laid out as rank
    lines: one 128-byte line per query) and the 8-lane kernels must give the oracle's answers on every block kind --
    NULL, FULL, bit, sparse and dense GAP -- incl. dead queries (rank 0, rank > count, position past the end) and
    batches that do not fill the last round"""
    c = bm.context(0)
    c.set_tuning("rs_lanes", unroll)
    c.set_tuning("rs_lines", 2 if lines else 0)                           # (2 = lines whatever the memory policy says: this vector is mostly NULL / FULL / GAP)
    # select over the lines: 1 = block index + octant directory (k_select_lines), 2 = select directory (k_select_sdir;
    # with 64 ones per entry -- several entries per line -- and with one entry for the whole vector: the bisection path)
    # a third element 1: the directory's 65,536-entry summary in LDS (k_select_top, round 5) forced for every batch size
    if isinstance(sel, tuple):
        c.set_tuning("rs_sdir_shift", sel[1])
        if len(sel) > 2: c.set_tuning("rs_select_top", sel[2])
        sel = sel[0]
    c.set_tuning("rs_select_lines", sel)
    # select lines (round 6, k_select_sel): 0 = not built, so that the forms above run the kernels they name; 1 = built with 16-bit
    # offsets -- this vector has NULL blocks, a line of 60 ones spans more than a block somewhere, so the build must notice and
    # take the 32-bit form; 2 = 32-bit offsets asked for; -1 = the memory policy decides
    c.set_tuning("rs_select_sel", selfmt)
    rng = np.random.default_rng(1234 + unroll)
    nbits, words = _rs_mixed_words(rng)
    p = port.import_words(words, True, nbits)
    assert set(p.flatten()[0].tolist()) == {0, 1, 2, 3}
    v = bm.bvector.from_block_table(c, nbits, *p.flatten())
    rs, prs = v.build_rs_index(), port.rs_build(p)
    cnt = p.count()
    if selfmt == 0: assert rs.info()["select_offset_bits"] == 0
    if selfmt > 0: assert rs.info()["select_offset_bits"] == 32 and rs.info()["select_lines_bytes"] == (cnt + 29) // 30 * 128
    for nq in (1, 7, 8, 9, 63, 1000, 4097):
        q = np.concatenate([rng.integers(0, nbits, size=nq).astype(np.uint64), np.array([0, nbits - 1, nbits, nbits + 70000, 65535, 65536], np.uint64)])
        assert (v.rank(q, rs) == prs.rank(q)).all(), (unroll, lines, nq)
        every = np.arange(max(0, int(q[0]) - 2000), min(nbits, int(q[0]) + 2000), dtype=np.uint64)    # every position around a query: all line / word borders
        assert (v.rank(every, rs) == prs.rank(every)).all(), (unroll, lines, nq)
        r = np.concatenate([rng.integers(1, cnt + 1, size=nq).astype(np.uint64), np.array([1, cnt, 0, cnt + 1, 2 ** 40], np.uint64)])
        found, pos = v.select(r, rs)
        ppos, pfound = prs.select(r)
        assert (found == pfound).all() and (pos[found] == ppos[pfound]).all(), (unroll, nq)
        assert (pos[~found] == 0).all()
    # every one of the vector, in order: select(k) must walk the set bits (all line borders, empty blocks in between)
    allr = np.arange(1, cnt + 1, dtype=np.uint64)[:: max(1, cnt // 200000)]
    found, pos = v.select(allr, rs)
    ppos, pfound = prs.select(allr)
    assert found.all() and (pos == ppos).all()
    del rs, v
    c.close()


@pytest.mark.parametrize("lines,selfmt", [(0, 0), (2, 0), (2, 1)])
def test_rank_select_automatic_choice(port, lines, selfmt):
    """rs_lanes 0: the library picks the lanes per query and the kernel from the batch size, the index and rs_sorted_hint.  Batches of
    65,535 and 65,536 queries (the threshold of the automatic lanes) over an index of tables only, one with rank lines and select
    directory, and one with select lines too; each with the sorted hint off and on (hinted batches are sorted as a whole, so their dead
    queries stand where ascending order puts them) and one hinted batch that is not ascending: the hint may cost time, never answers.
    Over the rank lines also 2^22 - 1 and 2^22 random ranks with rs_select_top -1: the threshold of k_select_top.  Every batch holds
    the dead queries (rank 0, count + 1, 2^40; positions nbits and nbits + 70000), unhinted ones at their end.  Expected values come
    from NumPy over the words; a few hundred queries of each kind also go against the oracle."""
    nbits, words, ones = _rs_mixed_reference()
    cnt = ones.size
    c = bm.context(0)
    for k, x in (("rs_lanes", 0), ("rs_lines", lines), ("rs_select_sel", selfmt), ("rs_select_top", -1)): c.set_tuning(k, x)
    p = port.import_words(np.array(words), True, nbits)
    assert p.count() == cnt
    v = bm.bvector.from_block_table(c, nbits, *p.flatten())
    rs = v.build_rs_index()
    info = rs.info()
    assert info["has_lines"] == bool(lines) and info["select_offset_bits"] == (32 if selfmt else 0)
    rng = np.random.default_rng(99 + lines + selfmt)
    dead_q, dead_r = np.array([nbits, nbits + 70000], np.uint64), np.array([0, cnt + 1, 2 ** 40], np.uint64)

    def batches(nq, hint):
        q = np.concatenate([rng.integers(0, nbits, size=nq - dead_q.size).astype(np.uint64), dead_q])
        r = np.concatenate([rng.integers(1, cnt + 1, size=nq - dead_r.size).astype(np.uint64), dead_r])
        return (np.sort(q), np.sort(r)) if hint else (q, r)

    for nq in (65535, 65536):
        for hint in (0, 1):
            c.set_tuning("rs_sorted_hint", hint)
            q, r = batches(nq, hint)
            assert q.size == nq and r.size == nq
            _check_rank_np(v, rs, ones, q, (nq, hint))
            _check_select_np(v, rs, ones, r, (nq, hint))
    c.set_tuning("rs_sorted_hint", 1)
    q, r = batches(65536, 0)                                               # hinted, not ascending
    _check_rank_np(v, rs, ones, q, "hinted, unsorted")
    _check_select_np(v, rs, ones, r, "hinted, unsorted")
    c.set_tuning("rs_sorted_hint", 0)
    if lines and not selfmt:
        for nq in ((1 << 22) - 1, 1 << 22):
            _check_select_np(v, rs, ones, batches(nq, 0)[1], nq)
    q, r = batches(300, 0)
    _check_against_oracle(v, rs, port.rs_build(p), q, r)
    del rs, v
    c.close()


def test_select_summary_dropped_when_groups_spread(port):
    """2,000 GAP blocks of three ones each: a select-directory entry covers 2^6 = 64 ones, a group of 64 summary entries 4,096 ones =
    1,365 blocks x 69 lines, more than the 65,000 lines a group may span even in whole lines (fb = 0).  bmx_rs_build must drop the
    directory's summary (k_select_top) although rs_select_top 1 asks for it, and select answers through the directory: the index's
    bytes are its tables, rank lines, octant directory and select directory, without the 135,168 bytes of a summary."""
    nblk, offs = 2000, np.array([5, 30000, 65000], np.int64)
    nbits = nblk * 65536
    words = np.zeros(nblk * 2048, np.uint32)
    for o in offs: words[np.arange(nblk) * 2048 + (o >> 5)] |= np.uint32(1 << (o & 31))
    ones = _ones_of(words, nbits)
    cnt = ones.size
    assert cnt == 3 * nblk
    c = bm.context(0)
    for k, x in (("rs_lines", 2), ("rs_select_sel", 0), ("rs_select_top", 1), ("rs_sdir_shift", 0)): c.set_tuning(k, x)
    p = port.import_words(words, True, nbits)
    assert set(p.flatten()[0].tolist()) == {3}                            # GAP blocks only
    v =bm.bvector.from_block_table(c, nbits, *p.flatten())
    rs = v.build_rs_index()
    sdir_entries = ((cnt + 63) >> 6) + 1
    assert rs.info() == {"bytes": nblk * (4 + 8 + 8 + 2 * 128) + nblk * 69 * 128 + nblk * 16 + sdir_entries * 4, "has_lines": True,
                         "select_offset_bits": 0, "select_lines_bytes": 0}
    rng = np.random.default_rng(7)
    dead_r = np.array([0, cnt + 1, 2 ** 40], np.uint64)
    _check_select_np(v, rs, ones, np.arange(1, cnt + 1, dtype=np.uint64), "in order")
    r = np.concatenate([rng.integers(1, cnt + 1, size=1000).astype(np.uint64), dead_r])
    _check_select_np(v, rs, ones, r, "random")
    _check_rank_np(v, rs, ones, ones, "at every one")
    _check_rank_np(v, rs, ones, ones + np.uint64(1), "behind every one")
    q = np.concatenate([rng.choice(ones, 98), rng.choice(ones, 98) + np.uint64(1), np.array([0, nbits - 1, nbits, nbits + 70000], np.uint64)])
    _check_against_oracle(v, rs, port.rs_build(p), q, r[-200:])
    del rs, v
    c.close()


@pytest.mark.parametrize("dq,nblk", [(6554, 40), (655, 40), (30000, 9), (200, 12)])
def test_select_lines_16_bit_form(port, dq, nblk):
    """select lines with 16-bit offsets (bmx_kernels11.h): a vector whose ones are spread evenly enough that 60 consecutive ones
    never span a whole block keeps the 16-bit form -- lines that straddle one, two block borders (low bits wrap), bit and GAP
    blocks, a FULL block in the middle; every one of the vector in order, random batches, dead queries.  At dq = 200
    (0.3 %: 60 ones span ~20,000 bits on average, sometimes > 65,535) either form may result; the answers must not change"""
    c = bm.context(0)
    c.set_tuning("rs_select_sel", 1)
    nbits = nblk * 65536 - 4321
    words = port.gen_words(777 + dq, 3, dq, nbits)
    words[5 * 2048:6 * 2048] = 0xFFFFFFFF                                 # one FULL block
    p = port.import_words(words, True, nbits)
    v = bm.bvector.from_block_table(c, nbits, *p.flatten())
    rs, prs = v.build_rs_index(), port.rs_build(p)
    cnt = p.count()
    info = rs.info()
    if dq >= 655: assert info["select_offset_bits"] == 16 and info["select_lines_bytes"] == (cnt + 59) // 60 * 128, info
    else: assert info["select_offset_bits"] in (16, 32)
    allr = np.arange(1, cnt + 1, dtype=np.uint64)
    if cnt > 400000: allr = allr[:: cnt // 400000 + 1]
    found, pos_all = v.select(allr, rs)
    ppos, pfound = prs.select(allr)
    assert found.all() and (pos_all == ppos).all()
    rng = np.random.default_rng(dq)
    for nq in (1, 63, 64, 65, 511, 512, 513, 100000):
        r = np.concatenate([rng.integers(1, cnt + 1, size=nq).astype(np.uint64), np.array([1, cnt, 0, cnt + 1, 2 ** 40, 60, 61, 120, 121], np.uint64)])
        found, pos = v.select(r, rs)
        ppos, pfound = prs.select(r)
        assert (found == pfound).all() and (pos[found] == ppos[pfound]).all() and (pos[~found] == 0).all(), (dq, nq)
    # the policy form: the same answers whether or not the index took the lines
    c.set_tuning("rs_select_sel", 0)
    f0, p0 = v.select(allr[:5000], rs)
    assert f0.all() and (p0 == pos_all[:5000]).all()
    del rs, v
    c.close()


@pytest.mark.parametrize("dq,nblk,uneven", [(32768, 300, False), (20000, 150, True), (6554, 400, False)])
def test_select_top_position_exact_summary(port, dq, nblk, uneven):
    """k_select_top with the round-6 summary (an entry = the position of its sampled one to 1 / 2^fb of a line, bases per 64 entries):
    dense vectors, which the select lines do not cover; an uneven vector (a stretch of empty blocks in the middle: the groups' spread
    decides fb); every answer against the oracle -- the headers decide, the summary only guesses"""
    c = bm.context(0)
    c.set_tuning("rs_select_sel", 0); c.set_tuning("rs_lines", 2); c.set_tuning("rs_select_top", 1)
    nbits = nblk * 65536 - 1234
    words = port.gen_words(4321 + dq, 9, dq, nbits)
    if uneven: words[40 * 2048:110 * 2048] = 0
    p = port.import_words(words, True, nbits)
    v = bm.bvector.from_block_table(c, nbits, *p.flatten())
    rs, prs = v.build_rs_index(), port.rs_build(p)
    cnt = p.count()
    rng = np.random.default_rng(dq)
    for nq in (1, 63, 5000, 300000):
        r = np.concatenate([rng.integers(1, cnt + 1, size=nq).astype(np.uint64), np.array([1, cnt, 0, cnt + 1], np.uint64)])
        found, pos = v.select(r, rs)
        ppos, pfound = prs.select(r)
        assert (found == pfound).all() and (pos[found] == ppos[pfound]).all() and (pos[~found] == 0).all(), (dq, nq)
    allr = np.arange(1, cnt + 1, dtype=np.uint64)[:: max(1, cnt // 250000)]
    found, pos = v.select(allr, rs)
    assert found.all() and (pos == prs.select(allr)[0]).all()
    del rs, v
    c.close()


def _sparse_collection(port, rng, nvec, nbits, dq, long_runs=False, ragged=False, specials=True):
    """GAP-only operands (no bit-blocks): sparse noise OR a shared component (so that ANDs survive), optionally wide
    1-runs (multi-word intervals), NULL / FULL blocks and operands shorter than the others"""
    nblk = (nbits + 65535) // 65536
    words = []
    common = port.gen_words(4242, 0xFFFFFFFF, max(dq // 2, 3), nbits)
    for v in range(nvec):
        nb = nbits
        if ragged and v % 7 == 3:
            nb = max(65536 - 99, nbits - (1 + v % 3) * 65536)
        w = port.gen_words(4242, v, dq, nb) | common[: ((nb + 63) // 64) * 2]
        nw = (nb + 31) // 32
        if nb % 32: w[nw - 1] &= np.uint32((1 << (nb % 32)) - 1)
        w[nw:] = 0
        if long_runs:
            for _ in range(6):
                a = int(rng.integers(0, nw - 40)); l = int(rng.integers(1, 40))
                w[a:a + l] = 0xFFFFFFFF
        if specials:
            for b in range(w.size // 2048):
                r = rng.integers(0, 30)
                if r == 0 and v % 11 == 5: w[b * 2048:(b + 1) * 2048] = 0                      # NULL block
                elif r == 1 and (b + 1) * 65536 <= nb: w[b * 2048:(b + 1) * 2048] = 0xFFFFFFFF   # FULL block
        words.append(w)
    return words


@pytest.mark.parametrize("dq,nvec,long_runs", [(13, 200, False), (150, 96, True), (280, 64, True), (30, 300, False)])
def test_packed_gap_collections(port, dq, nvec, long_runs):
    """combine_or / combine_and / combine_and_sub / one-group counts pipelines over GAP-only operand sets through the
    column-major packed collection (bmx_kernels6.h, gap_pack 1) must equal the oracle bit for bit AND block kind for
    block kind, and equal what the descriptor-table kernels (gap_pack 0) produce: NULL / FULL operands, operands of
    different lengths, single-bit runs, runs spanning many words, SUB lists of any size"""
    rng = np.random.default_rng(dq * 1000 + nvec)
    nbits = 6 * 65536 + 1234
    words = _sparse_collection(port, rng, nvec, nbits, dq, long_runs=long_runs, ragged=True)
    pv = [port.import_words(w, True, w.size * 32) for w in words]
    assert all(p.flatten()[0].tolist().count(2) == 0 for p in pv), "operands must be free of bit-blocks"
    nwb = 7 * 2048
    results = {}
    for mode in (1, 2, 0):                                             # packed with split bags (default) / packed with plain bags / table kernels
        c = bm.context(0)
        c.set_tuning("gap_pack", min(mode, 1)); c.set_tuning("coll_split", 1 if mode == 1 else 0)
        c.set_tuning("direct_cols", 0); c.set_tuning("pipe_split", 0)   # (few columns: keep the one-launch small-collection kernels out of the way)
        gv = [bm.bit_import_u32(c, w, True) for w in words]
        agg = bm.aggregator(c)
        out = []
        for opt in (False, True):
            agg.set_optimization(opt)
            o = agg.combine_or(gv)
            e = port.agg_or(pv, opt)
            assert (o.to_words(nwb) == e.to_words(nwb)).all(), (mode, opt)
            assert o.block_table()[0].tolist() == (e.flatten()[0].tolist() + [0] * 8)[:o.info()["nblocks"]], (mode, opt)
            out.append(o.block_table()[0].tolist())
        agg.set_optimization(False)
        half = nvec // 2
        for a, s in [(list(range(nvec)), []), (list(range(half)), list(range(half, nvec))), (list(range(0, nvec, 2)), [1, 3]),
                     (list(range(nvec - 64, nvec)), [0]), (list(range(64)), list(range(64, nvec)))]:
            t, any_ = agg.combine_and_sub([gv[i] for i in a], [gv[i] for i in s])
            e = port.agg_and_sub([pv[i] for i in a], [pv[i] for i in s])
            assert (t.to_words(nwb) == e.to_words(nwb)).all(), (mode, len(a), len(s))
            assert t.block_table()[0].tolist() == (e.flatten()[0].tolist() + [0] * 8)[:t.info()["nblocks"]], (mode, len(a), len(s))
            assert any_ == (e.count() > 0)
            pipe = bm.aggregator.pipeline(c)
            ag = pipe.add()
            for i in a: ag.add(gv[i], 0)
            for i in s: ag.add(gv[i], 1)
            pipe.complete()
            assert int(agg.combine_and_sub(pipe)[0]) == e.count(), (mode, len(a), len(s))
            assert int(agg._run_pipeline(pipe, 1, 4)[0]) == int(port.pipeline_counts([([pv[i] for i in a], [pv[i] for i in s])], 1, 4)[0])
            out.append(t.block_table()[0].tolist())
        st = c.pack_stats()
        assert (st["collections"] > 0) == (mode >= 1), st
        results[mode] = out
        if mode >= 1:
            # a freed operand takes the collections that hold its runs with it
            before = c.pack_stats()["collections"]
            del o, t, pipe, ag
            agg.reset()
            g0 = gv.pop(0)
            assert c.pack_stats()["collections"] == before
            del g0
            import gc; gc.collect()
            assert c.pack_stats()["collections"] < before
        del gv
        c.close()
    assert results[0] == results[1] == results[2]


@pytest.mark.parametrize("dq,nvec,long_runs,nblk", [(13, 200, False, 40), (13, 1100, False, 19), (150, 96, True, 35), (30, 300, True, 7), (3, 70, False, 33)])
def test_combine_or_row_kernel(port, dq, nvec, long_runs, nblk):
    """combine_or over >= 64 GAP-only operands through the tile directories (k_agg_or_rows, bmx_kernels7.h; or_rows 1, both
    depths) = the oracle bit for bit, block kind for block kind (with and without the aggregator's optimisation), with the
    popcount the kernel folds, and = the column-tile kernel (or_rows 0): sparse rows (<= 64 chunks per tile), tiles the
    directory hands to the descriptor path (dense GAP blocks, FULL blocks), NULL columns inside a tile, operands shorter
    than the others, more than 1,024 operands (a wave's second batch of records), a partial last tile"""
    rng = np.random.default_rng(dq * 977 + nvec)
    nbits = nblk * 65536 - 4321
    words = _sparse_collection(port, rng, nvec, nbits, dq, long_runs=long_runs, ragged=True)
    for v in range(0, nvec, 9):                                        # whole stretches of NULL blocks (NULL columns inside tiles)
        b0 = int(rng.integers(0, nblk - 1)); b1 = min(nblk, b0 + int(rng.integers(1, 6)))
        words[v][b0 * 2048:b1 * 2048] = 0
    pv = [port.import_words(w, True, w.size * 32) for w in words]
    assert all(p.flatten()[0].tolist().count(2) == 0 for p in pv), "operands must be free of bit-blocks"
    nwb = (nblk + 1) * 2048
    tables = {}
    for mode, depth in ((1, 4), (1, 8), (0, 4)):
        c = bm.context(0)
        c.set_tuning("gap_pack", 0); c.set_tuning("direct_cols", 0); c.set_tuning("pipe_split", 0)
        c.set_tuning("or_rows", mode); c.set_tuning("or_depth", depth)
        gv = [bm.bit_import_u32(c, w, True) for w in words]
        agg = bm.aggregator(c)
        out = []
        for opt in (False, True):
            agg.set_optimization(opt)
            for sel in (slice(None), slice(3, 3 + 64), slice(1, None, 2)):
                o = agg.combine_or(gv[sel])
                e = port.agg_or(pv[sel], opt)
                assert (o.to_words(nwb) == e.to_words(nwb)).all(), (mode, depth, opt, sel)
                assert o.block_table()[0].tolist() == (e.flatten()[0].tolist() + [0] * 8)[:o.info()["nblocks"]], (mode, depth, opt, sel)
                assert o.count() == e.count(), (mode, depth, opt, sel)
                assert bm.count_xor(o, o) == 0 and bm.count_and(o, o) == e.count()
                out.append(o.block_table()[0].tolist())
        tables[(mode, depth)] = out
        del gv, o
        c.close()
    assert tables[(1, 4)] == tables[(1, 8)] == tables[(0, 4)]


def test_packed_collection_policy_and_prepare(port):
    """gap_pack -1 (default): collections exist only where bmx_collection_prepare built them -- no aggregation builds one on
    the side; gap_pack 1: the first use of a list of >= 64 packable vectors builds its collection; results never depend on
    which path ran"""
    rng = np.random.default_rng(77)
    nbits = 4 * 65536
    words = _sparse_collection(port, rng, 80, nbits, 40, specials=False)
    pv = [port.import_words(w, True, nbits) for w in words]
    c = bm.context(0)
    c.set_tuning("direct_cols", 0); c.set_tuning("pipe_split", 0)
    gv = [bm.bit_import_u32(c, w, True) for w in words]
    agg = bm.aggregator(c)
    e = port.agg_or(pv)
    o1 = agg.combine_or(gv)
    o2 = agg.combine_or(gv)
    assert c.pack_stats()["collections"] == 0                # default policy: nothing is built behind the caller's back
    c.collection_prepare(gv, bm.ROLE_OR)
    st = c.pack_stats()
    assert st["collections"] == 1 and st["bytes"] > 0 and st["last_build_ms"] > 0
    c.collection_prepare(gv, bm.ROLE_OR)                      # the same list in the same role: already there
    assert c.pack_stats()["collections"] == 1
    o3 = agg.combine_or(gv)
    o4 = agg.combine_or(gv[::-1])                             # any order
    o5 = agg.combine_or(gv + gv[:7])                          # repeats
    assert c.pack_stats()["collections"] == 1
    for o in (o1, o2, o3, o4, o5):
        assert (o.to_words() == e.to_words(o.info()["nblocks"] * 2048)).all()
    c.collection_prepare(gv, bm.ROLE_AND)
    assert c.pack_stats()["collections"] == 2
    t, _ = agg.combine_and_sub(gv, [])
    assert c.pack_stats()["collections"] == 2
    assert (t.to_words() == port.agg_and_sub(pv, []).to_words(t.info()["nblocks"] * 2048)).all()
    c.collection_prepare(gv[:10], bm.ROLE_OR)                 # a small collection is a collection too
    assert c.pack_stats()["collections"] == 3
    dense = bm.bit_import_u32(c, port.gen_words(1, 1, 30000, nbits), True)
    with pytest.raises(bm.BmxError):
        c.collection_prepare(gv + [dense], bm.ROLE_OR)     # bit-blocks cannot be packed
    del gv, o1, o2, o3, o4, o5, t, dense
    c.close()
    # gap_pack 1: built at first use
    c = bm.context(0)
    c.set_tuning("direct_cols", 0); c.set_tuning("pipe_split", 0); c.set_tuning("gap_pack", 1)
    gv = [bm.bit_import_u32(c, w, True) for w in words]
    agg = bm.aggregator(c)
    o1 = agg.combine_or(gv)
    assert c.pack_stats()["collections"] == 1
    assert (o1.to_words() == e.to_words(o1.info()["nblocks"] * 2048)).all()
    del gv, o1
    c.close()


def test_packed_collection_budget(port, monkeypatch):
    """the packing budget (a quarter of the free HBM at context creation; BMX_PACK_MAX_MB): a collection that does not fit is
    refused with BMX_ERR_BADALLOC and nothing else changes; collections that fit one at a time push the least recently used
    one out; aggregations keep answering the same through whichever path is left"""
    rng = np.random.default_rng(5)
    nbits = 48 * 65536
    words = _sparse_collection(port, rng, 240, nbits, 80, specials=False)
    pv = [port.import_words(w, True, nbits) for w in words]
    monkeypatch.setenv("BMX_PACK_MAX_MB", "1")
    c = bm.context(0)
    try:
        c.set_tuning("direct_cols", 0); c.set_tuning("pipe_split", 0)
        gv = [bm.bit_import_u32(c, w, True) for w in words]
        agg = bm.aggregator(c)
        e_all = port.agg_or(pv, False)
        with pytest.raises(bm.BmxError):                       # 240 vectors x 48 columns x ~120 runs: 5 MB of run lists
            c.collection_prepare(gv, bm.ROLE_OR)
        assert c.pack_stats()["collections"] == 0
        o = agg.combine_or(gv)
        assert (o.to_words() == e_all.to_words(o.info()["nblocks"] * 2048)).all()
        parts = [gv[0:30], gv[30:60], gv[60:90], gv[90:120]]
        for k, part in enumerate(parts):                       # each ~0.35 MB (0.7 MB of GAP words: under the budget): two fit, the next one pushes the least recently used one out
            c.collection_prepare(part, bm.ROLE_OR)
            st = c.pack_stats()
            assert 1 <= st["collections"] <= 2 and st["bytes"] <= (1 << 20), (k, st)
        for k, part in enumerate(parts):                       # every part still aggregates to the oracle's bits (packed or not)
            o = agg.combine_or(part)
            e = port.agg_or(pv[30 * k:30 * k + 30], False)
            assert (o.to_words() == e.to_words(o.info()["nblocks"] * 2048)).all(), k
        del gv, o, agg
    finally:
        c.close()


@pytest.mark.parametrize("dq,nvec,long_runs,nblk", [(13, 300, False, 9), (150, 120, True, 6), (40, 1100, False, 3)])
def test_prepared_collection_subsets_and_pipelines(port, dq, nvec, long_runs, nblk):
    """ONE prepared collection per role serves any later aggregation over its vectors (member directory, bmx_kernels8.h):
    combine_or / combine_and_sub over 20 random subsets in random order (with repeats), a 64-group counts pipeline and a
    64-group results pipeline (AND lists and SUB lists drawn from the collection's vectors) = the oracle's bits, block
    kinds and counts, = what the descriptor-table kernels give (gap_pack 0), and no further collection is built"""
    rng = np.random.default_rng(dq * 31 + nvec)
    nbits = nblk * 65536 - 1234
    words = _sparse_collection(port, rng, nvec, nbits, dq, long_runs=long_runs, ragged=True)
    pv = [port.import_words(w, True, w.size * 32) for w in words]
    assert all(p.flatten()[0].tolist().count(2) == 0 for p in pv), "operands must be free of bit-blocks"
    nwb = (nblk + 1) * 2048
    subsets = []
    for k in range(20):
        m = int(rng.integers(16, nvec))
        sel = rng.choice(nvec, size=m, replace=(k % 5 == 4)).tolist()
        subsets.append(sel)
    groups = []
    for g in range(64):
        na = int(rng.integers(1, 4)) if g % 8 else int(rng.integers(20, 60))
        ns = int(rng.integers(0, 40))
        a = rng.choice(nvec, size=na, replace=False).tolist()
        s_ = [i for i in rng.choice(nvec, size=ns, replace=False).tolist() if i not in a]
        groups.append((a, s_))
    groups[5] = (groups[5][0], [])                                         # no SUB list
    outs = {}
    for mode in ("prepared", "tables"):
        c = bm.context(0)
        c.set_tuning("direct_cols", 0); c.set_tuning("pipe_split", 0)
        if mode == "tables": c.set_tuning("gap_pack", 0)
        else: c.set_tuning("coll_members", 1)                              # (always through the member directory, also where the tables would be picked)
        gv = [bm.bit_import_u32(c, w, True) for w in words]
        if mode == "prepared":
            c.collection_prepare(gv, bm.ROLE_OR)                           # polarity 1: OR lists and SUB lists
            c.collection_prepare(gv, bm.ROLE_AND)                          # polarity 0: AND lists
            ncoll = c.pack_stats()["collections"]
            assert ncoll == 2
        agg = bm.aggregator(c)
        out = []
        for k, sel in enumerate(subsets):
            opt = bool(k & 1)
            agg.set_optimization(opt)
            o = agg.combine_or([gv[i] for i in sel])
            e = port.agg_or([pv[i] for i in sel], opt)
            assert (o.to_words(nwb) == e.to_words(nwb)).all(), (mode, k)
            assert o.block_table()[0].tolist() == (e.flatten()[0].tolist() + [0] * 8)[:o.info()["nblocks"]], (mode, k)
            out.append(o.block_table()[0].tolist())
            agg.set_optimization(False)
            half = len(sel) // 3
            t, any_ = agg.combine_and_sub([gv[i] for i in sel[:half]], [gv[i] for i in sel[half:]])
            e = port.agg_and_sub([pv[i] for i in sel[:half]], [pv[i] for i in sel[half:]])
            assert (t.to_words(nwb) == e.to_words(nwb)).all(), (mode, k)
            assert t.block_table()[0].tolist() == (e.flatten()[0].tolist() + [0] * 8)[:t.info()["nblocks"]], (mode, k)
            assert any_ == (e.count() > 0)
            out.append(t.block_table()[0].tolist())
        # 64 arg-groups, counts only
        pipe = bm.aggregator.pipeline(c)
        for a, s_ in groups:
            ag = pipe.add()
            for i in a: ag.add(gv[i], 0)
            for i in s_: ag.add(gv[i], 1)
        pipe.complete()
        got = [int(x) for x in agg.combine_and_sub(pipe)]
        exp = [port.agg_and_sub([pv[i] for i in a], [pv[i] for i in s_]).count() for a, s_ in groups]
        assert got == exp, mode
        if mode == "prepared": assert "k_coll_members" in pipe.describe(), pipe.describe()
        part = [int(x) for x in agg._run_pipeline(pipe, 1, max(2, nblk - 1))]
        assert part == [int(x) for x in port.pipeline_counts([([pv[i] for i in a], [pv[i] for i in s_]) for a, s_ in groups], 1, max(2, nblk - 1))], mode
        # 64 arg-groups, result vectors + counts
        pipe2 = bm.aggregator.pipeline(c, bm.agg_run_options(True, True))
        for a, s_ in groups:
            ag = pipe2.add()
            for i in a: ag.add(gv[i], 0)
            for i in s_: ag.add(gv[i], 1)
        pipe2.complete()
        agg.combine_and_sub(pipe2)
        assert [int(x) for x in pipe2.get_bv_count_vector()] == exp, mode
        for (a, s_), r in zip(groups, pipe2.get_bv_res_vector()):
            e = port.agg_and_sub([pv[i] for i in a], [pv[i] for i in s_])
            if e.count() == 0:
                assert r is None
                continue
            assert (r.to_words(nwb) == e.to_words(nwb)).all(), mode
            assert r.block_table()[0].tolist() == (e.flatten()[0].tolist() + [0] * 8)[:r.info()["nblocks"]], mode
        if mode == "prepared": assert c.pack_stats()["collections"] == ncoll      # nothing was built on the side
        outs[mode] = out
        del gv, o, t, pipe, pipe2, ag
        c.close()
    assert outs["prepared"] == outs["tables"]


# ---- round-3 fixtures generated by the reference: set_range_hint and the sparse_vector_scanner ----
@pytest.mark.parametrize("case", list(CASES))
def test_range_hint_vs_reference_golden(ctx, port, golden, case):
    """aggregator::set_range_hint (src/bmaggregator.h:481,974): find_first_and_sub under a hint and a pipeline whose options
    enable search masks (agg_run_options<true, true, true>, :1312-1346) against what the live bm::aggregator returned
    (tests/golden/make_golden.py): counts, result presence, content and block kinds per arg-group"""
    from cases import HINT_GROUPS, range_hints
    g = golden["cases"][case]
    words, nbits = make_inputs(port, case)
    gv = [bm.bit_import_u32(ctx, w, True) for w in words]
    for v, w in zip(gv, words):
        assert v.info()["nbits"] >= nbits - 63
    nblk = (nbits + 65535) // 65536
    agg = bm.aggregator(ctx)
    for (frm, to), e in zip(range_hints(nbits), g["range_hint"]):
        assert (e["from"], e["to"]) == (frm, to)
        one = agg.set_range_hint(frm, to)
        for gi, (a, s) in enumerate(HINT_GROUPS):
            ff = e["find_first"][gi]
            assert one == ff["hint_one_block"]
            found, idx = agg.find_first_and_sub([gv[i] for i in a], [gv[i] for i in s])
            assert found == ff["found"] and (not found or idx == ff["idx"]), (case, frm, to, gi)
        pipe = bm.aggregator.pipeline(ctx, bm.agg_run_options(True, True, True))
        for a, s in HINT_GROUPS:
            ag = pipe.add()
            for i in a: ag.add(gv[i], 0)
            for i in s: ag.add(gv[i], 1)
        pipe.complete()
        agg.combine_and_sub(pipe)
        assert [int(x) for x in pipe.get_bv_count_vector()] == e["counts"], (case, frm, to)
        res = pipe.get_bv_res_vector()
        assert [r is not None for r in res] == e["present"], (case, frm, to)
        for gi, r in enumerate(res):
            if r is None: continue
            assert sha(r.to_words(nblk * 2048)) == e["sha"][gi], (case, frm, to, gi)
            assert r.block_table()[0].tolist() == (e["kinds"][gi] + [0] * nblk)[:r.info()["nblocks"]], (case, frm, to, gi)
        # counts-only pipeline with masks under the same hint
        p2 = bm.aggregator.pipeline(ctx, bm.agg_run_options(False, True, True))
        for a, s in HINT_GROUPS:
            ag = p2.add()
            for i in a: ag.add(gv[i], 0)
            for i in s: ag.add(gv[i], 1)
        p2.complete()
        assert [int(x) for x in agg.combine_and_sub(p2)] == e["counts"], (case, frm, to)
        agg.reset_range_hint()


@pytest.mark.parametrize("with_null", [False, True])
def test_slice_scanner_vs_reference_golden(ctx, golden, with_null):
    """bmx slice_scanner over bit-planes built by numpy from cases.scanner_values against the result vectors of the real
    bm::sparse_vector_scanner<> (tests/golden/golden_ref.json "scanner"): find_gt / ge / lt / le / range / eq / zero /
    nonzero (content + counts), find_first_eq, and a batch of equality counts through both batch paths"""
    from cases import SCANNER_EQ_BATCH, SCANNER_RANGES, SCANNER_ROWS, SCANNER_VALUES, scanner_values
    g = golden["scanner"]["with_null" if with_null else "no_null"]
    n = SCANNER_ROWS
    vals, isn = scanner_values(with_null)
    assert sha(vals) == g["values_sha"]
    def upload(bits):
        w = np.packbits(np.concatenate([bits.astype(np.uint8), np.zeros((-n) % 32, np.uint8)]), bitorder="little").view(np.uint32)
        return bm.bit_import_u32(ctx, w, True)
    col = vals.astype(np.uint64)
    planes = []
    for i in range(g["effective_slices"]):
        bits = ((col >> np.uint64(i)) & np.uint64(1)) != 0
        planes.append(upload(bits) if bits.any() else None)
        assert g["plane_counts"][i] in (None, int(bits.sum())) and (planes[-1] is None) == (g["plane_counts"][i] in (None, 0))
    nn = upload(isn == 0) if with_null else None
    sc = bm.slice_scanner(ctx, planes, size=n, not_null=nn)
    nw = (n + 31) // 32
    def chk(t, e):
        assert t.count() == e["count"] and sha(t.to_words(nw)) == e["sha"], e
    for halves in (1, 0):
        ctx.set_tuning("range_halves", halves)
        for name, fn, pred in (("gt", sc.find_gt, bm.CMP_GT), ("ge", sc.find_ge, bm.CMP_GE), ("lt", sc.find_lt, bm.CMP_LT), ("le", sc.find_le, bm.CMP_LE)):
            for e in g["cmp"][name]:
                chk(fn(e["v"]), e)
                assert sc.count(pred, e["v"]) == e["count"]
        for e in g["range"]:
            chk(sc.find_range(e["from"], e["to"]), e)
            assert sc.count(bm.CMP_RANGE, e["from"], e["to"]) == e["count"]
        chk(sc.find_zero(), g["zero"]); chk(sc.find_nonzero(), g["nonzero"])
    ctx.set_tuning("range_halves", 1)
    for e, f in zip(g["cmp"]["eq"], g["eq_first"]):
        t, found = sc.find_eq(e["v"])
        assert found == (e["count"] > 0)
        if t is not None: chk(t, e)
        else: assert e["count"] == 0
        ff = sc.find_first_eq(e["v"]) if e["v"] else (f["found"], f["pos"])      # (value 0 has no AND group: find_eq(0) above covers it)
        assert ff[0] == f["found"] and (not f["found"] or ff[1] == f["pos"]), f
    for method in ("auto", "pipeline", "transpose"):
        try:
            got = sc.find_eq_counts(np.array(SCANNER_EQ_BATCH, np.uint64), method=method)
        except (TypeError, ValueError):
            continue
        assert [int(x) for x in got] == g["eq_counts"], method


def test_index_list_output(ctx, port):
    """bmx_vec_to_indices / combine_and_sub_bi / find_eq(value, BII): the result as SORTED positions (device compaction:
    per-block popcounts, running sum, per-word expansion) equals the set bits of the vector -- NULL, FULL, bit, sparse
    and dense GAP blocks, 32- and 64-bit positions, the empty vector, a buffer that is too small"""
    import ctypes as C
    from bitmagic_amd import _ffi
    rng = np.random.default_rng(31)
    nblk = 9
    nbits = nblk * 65536 - 4000
    words = np.zeros(nblk * 2048, np.uint32)
    words[2048:4096] = 0xFFFFFFFF                                                         # FULL
    words[2 * 2048:3 * 2048] = rng.integers(0, 1 << 32, 2048, dtype=np.uint64).astype(np.uint32)       # bit
    for b in rng.integers(3 * 65536, 4 * 65536, 50): words[b >> 5] |= np.uint32(1 << (b & 31))         # sparse GAP
    words[4 * 2048 + 100:4 * 2048 + 1900] = 0xFFFFFFFF                                   # wide run (GAP)
    words[6 * 2048:7 * 2048] = 0xFFFFFFFF; words[6 * 2048 + 7] = 0xFFFF7FFF               # nearly full (GAP, dense)
    for b in rng.integers(8 * 65536, nbits, 3000): words[b >> 5] |= np.uint32(1 << (b & 31))           # last, partial block
    p = port.import_words(words, True, nbits)
    assert set(p.flatten()[0].tolist()) == {0, 1, 2, 3}
    v = bm.bvector.from_block_table(ctx, nbits, *p.flatten())
    exp = np.flatnonzero(np.unpackbits(words.view(np.uint8), bitorder="little")).astype(np.uint64)
    got = v.to_indices()
    assert got.dtype == np.uint64 and (got == exp).all() and got.size == p.count()
    got32 = v.to_indices(4)
    assert got32.dtype == np.uint32 and (got32 == exp.astype(np.uint32)).all()
    # too small a buffer: nothing is written, the needed size comes back
    n = C.c_uint64()
    buf = np.zeros(10, np.uint64)
    rc = _ffi.lib().bmx_vec_to_indices(ctx._h, v._h, 8, buf.ctypes.data_as(C.c_void_p), 10, C.byref(n))
    assert rc == _ffi.ERR_RANGE and n.value == exp.size and not buf.any()
    empty = bm.bit_import_u32(ctx, np.zeros(4096, np.uint32), True)
    assert empty.to_indices().size == 0
    # aggregator: AND-SUB as positions
    ws = [port.gen_words(777, i, 3000, nbits) | port.gen_words(777, 0xFFFFFFFF, 2000, nbits) for i in range(5)]
    gv = [bm.bit_import_u32(ctx, w, True) for w in ws]
    pv = [port.import_words(w, True, w.size * 32) for w in ws]
    agg = bm.aggregator(ctx)
    e = port.agg_and_sub(pv[:3], pv[3:])
    ebits = np.flatnonzero(np.unpackbits(e.to_words(gv[0].info()["nblocks"] * 2048).view(np.uint8), bitorder="little"))
    assert (agg.combine_and_sub_bi(gv[:3], gv[3:]) == ebits.astype(np.uint64)).all() and ebits.size > 0
    agg.add(gv[0]); agg.add(gv[1]); agg.add(gv[4], 1)
    e2 = port.agg_and_sub(pv[:2], pv[4:])
    assert agg.combine_and_sub_bi().size == e2.count()
    assert agg.combine_and_sub_bi([gv[0], empty], []).size == 0
    # scanner: rows equal to a value as indices
    col = rng.integers(0, 50, 3 * 65536 + 99).astype(np.uint64)
    def upload(bits):
        w = np.packbits(np.concatenate([bits.astype(np.uint8), np.zeros((-col.size) % 32, np.uint8)]), bitorder="little").view(np.uint32)
        return bm.bit_import_u32(ctx, w, True)
    sc = bm.slice_scanner(ctx, [upload(((col >> np.uint64(i)) & np.uint64(1)) != 0) for i in range(6)], size=col.size)
    for val in (0, 1, 17, 49, 50, 63):
        assert (sc.find_eq_indices(val) == np.flatnonzero(col == val).astype(np.uint64)).all(), val


@pytest.mark.parametrize("with_null", [False, True])
def test_signed_scanner_inlist_invert_vs_reference_golden(ctx, golden, with_null):
    """bmx_slice_compare_signed (sign plane + magnitude planes, one pass), IN-list find_eq (pipeline with an OR target) and
    invert against the reference-generated fixtures: bm::sparse_vector_scanner<sparse_vector<int>> results incl. INT_MIN /
    INT_MAX bounds, ranges across zero, NULL rows; both kernel shapes (half-block passes and whole blocks)"""
    from cases import (SCANNER_IN_LISTS, SCANNER_ROWS, s2u, scanner_values, scanner_values_signed)
    n = SCANNER_ROWS
    nw = (n + 31) // 32
    def upload(bits):
        w = np.packbits(np.concatenate([bits.astype(np.uint8), np.zeros((-n) % 32, np.uint8)]), bitorder="little").view(np.uint32)
        return bm.bit_import_u32(ctx, w, True)
    def chk(t, e):
        assert t.count() == e["count"] and sha(t.to_words(nw)) == e["sha"], e
    g = golden["scanner"]["signed_with_null" if with_null else "signed_no_null"]
    vals, isn = scanner_values_signed(with_null)
    assert sha(vals) == g["values_sha"]
    u = s2u(vals)
    planes = []
    for i in range(g["effective_slices"]):
        bits = ((u >> np.uint64(i)) & np.uint64(1)) != 0
        planes.append(upload(bits) if bits.any() else None)
    nn = upload(isn == 0) if with_null else None
    sc = bm.slice_scanner(ctx, planes, size=n, not_null=nn, signed=True)
    for halves in (1, 0):
        ctx.set_tuning("range_halves", halves)
        for name, fn, pred in (("gt", sc.find_gt, bm.CMP_GT), ("ge", sc.find_ge, bm.CMP_GE), ("lt", sc.find_lt, bm.CMP_LT),
                               ("le", sc.find_le, bm.CMP_LE)):
            for e in g["cmp"][name]:
                chk(fn(e["v"]), e)
                assert sc.count(pred, e["v"]) == e["count"], (name, e["v"])
        for e in g["cmp"]["eq"]:
            assert sc.count(bm.CMP_EQ, e["v"]) == e["count"]
            chk(sc._compare(bm.CMP_EQ, e["v"]), e)
            t, found = sc.find_eq(e["v"])                       # the public call takes the signed value as well
            assert found == (e["count"] > 0), e
            if t is not None: chk(t, e)
            else: assert e["count"] == 0, e
        for e in g["range"]:
            chk(sc.find_range(e["from"], e["to"]), e)
            assert sc.count(bm.CMP_RANGE, e["from"], e["to"]) == e["count"]
        chk(sc.find_zero(), g["zero"]); chk(sc.find_nonzero(), g["nonzero"])
    ctx.set_tuning("range_halves", 1)
    # unsigned container: IN-list and invert
    gu = golden["scanner"]["with_null" if with_null else "no_null"]
    uv, uisn = scanner_values(with_null)
    col = uv.astype(np.uint64)
    uplanes = []
    for i in range(gu["effective_slices"]):
        bits = ((col >> np.uint64(i)) & np.uint64(1)) != 0
        uplanes.append(upload(bits) if bits.any() else None)
    usc = bm.slice_scanner(ctx, uplanes, size=n, not_null=upload(uisn == 0) if with_null else None)
    for e, lst in zip(gu["in_list"], SCANNER_IN_LISTS):
        chk(usc.find_eq_in(lst), e)
    # OR-ed into an existing vector, as the reference does
    pre = usc.find_gt(96)
    t = usc.find_eq_in([1, 2, 3], pre)
    exp = (col > 96) | np.isin(col, [1, 2, 3])
    assert t.count() == int(exp.sum())
    chk(usc.invert(usc.find_gt(50)), gu["invert_gt50"])
    # the plane bytes a range search actually reads are at most all of them and at least the top plane
    cnt, pb = usc.compare_stat(bm.CMP_GT, 50)
    assert cnt == int((col > 50).sum())
    total = sum(p.operand_bytes() for p in uplanes if p is not None)
    assert 0 < pb <= total


def test_pairwise_count_long_mixed_vectors(ctx, port):
    """bm::count_and/or/xor/sub over long vectors (> 2,048 blocks) of ANY block kinds vs the oracle: bit / sparse GAP /
    dense GAP / long runs / > 1,023-word GAP blocks / NULL / FULL on either side, operands of different lengths"""
    rng = np.random.default_rng(4711)
    nblk_a, nblk_b = 2300, 2177
    def build(nblk, seed):
        w = port.gen_words(9001, seed, 655, nblk * 65536)                      # 1 %: bit / GAP mix
        for nb in range(nblk):
            r = rng.integers(0, 12)
            lo = nb * 2048
            if r == 0: w[lo:lo + 2048] = 0
            elif r == 1: w[lo:lo + 2048] = 0xFFFFFFFF
            elif r == 2:                                                        # long runs -> GAP with wide 1-runs
                w[lo:lo + 2048] = 0; w[lo + 10:lo + 700] = 0xFFFFFFFF; w[lo + 1200:lo + 1210] = 0xFFFFFFFF; w[lo + 2047] = 0x80000000
            elif r == 3:                                                        # ~1,100 runs: a GAP block longer than 1,023 words
                w[lo:lo + 2048] = 0
                for b in rng.choice(65536, 560, replace=False): w[lo + (b >> 5)] |= np.uint32(1 << (b & 31))
            elif r == 4: w[lo:lo + 2048] = ~w[lo:lo + 2048]                     # dense: 0-runs are the short ones
            elif r == 5: w[lo:lo + 2048] = rng.integers(0, 1 << 32, 2048, dtype=np.uint64).astype(np.uint32)
        return w
    wa, wb = build(nblk_a, 1), build(nblk_b, 2)
    pa, pb = port.import_words(wa, True, wa.size * 32), port.import_words(wb, True, wb.size * 32)
    ka, kb = pa.flatten()[0], pb.flatten()[0]
    assert set(ka.tolist()) == {0, 1, 2, 3} and set(kb.tolist()) == {0, 1, 2, 3}
    assert max(int(x) for x in pa.flatten()[3][::1][:1]) >= 0
    ga, gb = bm.bvector.from_block_table(ctx, wa.size * 32, *pa.flatten()), bm.bvector.from_block_table(ctx, wb.size * 32, *pb.flatten())
    exp = [[port.count_op2(op, x, y) for op in range(4)] for x, y in ((pa, pb), (pb, pa), (pa, pa))]
    try:
        for pl in (0, 2, 3, 4, -1):              # a wave per column / the persistent kernel at 2, 3, 4 waves per SIMD / default
            ctx.set_tuning("pair_loop", pl)
            got = [[bm._count_op2(op, x, y) for op in range(4)] for x, y in ((ga, gb), (gb, ga), (ga, ga))]
            assert got == exp, (pl, got, exp)
    finally:
        ctx.set_tuning("pair_loop", -1)
    assert ga.count() == pa.count()


def test_pairwise_materialised_long_mixed_vectors(ctx, port):
    """bit_and/or/xor/sub over long vectors (> 2,048 blocks) of ANY block kinds: the persistent kernel (k_op2_loop, 2 / 4 / 8
    workgroups per CU, plain and non-temporal loads) and the wave-per-column kernel (op2_loop 0) = the oracle's bits AND block
    kinds, with and without opt_compress: bit / sparse GAP / dense GAP / long runs / > 1,023-word GAP blocks / NULL / FULL on
    either side, operands of different lengths"""
    rng = np.random.default_rng(1234)
    nblk_a, nblk_b = 2200, 2101
    def build(nblk, seed):
        w = port.gen_words(9002, seed, 655, nblk * 65536)                      # 1 %: bit / GAP mix
        for nb in range(nblk):
            r = rng.integers(0, 12)
            lo = nb * 2048
            if r == 0: w[lo:lo + 2048] = 0
            elif r == 1: w[lo:lo + 2048] = 0xFFFFFFFF
            elif r == 2:
                w[lo:lo + 2048] = 0; w[lo + 10:lo + 700] = 0xFFFFFFFF; w[lo + 1200:lo + 1210] = 0xFFFFFFFF; w[lo + 2047] = 0x80000000
            elif r == 3:
                w[lo:lo + 2048] = 0
                for b in rng.choice(65536, 560, replace=False): w[lo + (b >> 5)] |= np.uint32(1 << (b & 31))
            elif r == 4: w[lo:lo + 2048] = ~w[lo:lo + 2048]
            elif r == 5: w[lo:lo + 2048] = rng.integers(0, 1 << 32, 2048, dtype=np.uint64).astype(np.uint32)
        return w
    wa, wb = build(nblk_a, 1), build(nblk_b, 2)
    pa, pb = port.import_words(wa, True, wa.size * 32), port.import_words(wb, True, wb.size * 32)
    assert set(pa.flatten()[0].tolist()) == {0, 1, 2, 3} and set(pb.flatten()[0].tolist()) == {0, 1, 2, 3}
    ga, gb = bm.bvector.from_block_table(ctx, wa.size * 32, *pa.flatten()), bm.bvector.from_block_table(ctx, wb.size * 32, *pb.flatten())
    nw = max(wa.size, wb.size)
    exp = {}
    for opt in (0, 1):
        for op in range(4):
            for name, (x, y) in (("ab", (pa, pb)), ("ba", (pb, pa))):
                e = port.op2(op, x, y, opt)
                exp[(opt, op, name)] = (e.flatten()[0].tolist(), e.to_words(nw), e.count())
    try:
        for loop, nt in ((0, 3), (2, 3), (4, 2), (8, 3), (-1, 3), (-1, 0)):
            ctx.set_tuning("op2_loop", loop); ctx.set_tuning("op2_nt", nt)
            for opt in (0, 1):
                for op in range(4):
                    for name, (x, y) in (("ab", (ga, gb)), ("ba", (gb, ga))):
                        t = bm.bvector._op2(op, x, y, bm.opt_compress if opt else bm.opt_none)
                        kinds, words, cnt = exp[(opt, op, name)]
                        assert t.block_table()[0].tolist() == kinds, (loop, nt, opt, op, name)
                        assert (t.to_words(nw) == words).all(), (loop, nt, opt, op, name)
                        assert t.count() == cnt
                        if loop in (-1, 0) and name == "ab":
                            # the result as a host block table (GAP blocks laid out by the kernel in arrival order, ordinals of the
                            # kept bit slab computed at this first download) and back: same vector; and as an operand of later
                            # operations (its clone, a count against itself, an OR with an operand)
                            k2, o2, b2, g2 = t.block_table()
                            back = bm.bvector.from_block_table(ctx, t.info()["nbits"], k2, o2, b2, g2)
                            assert bm.count_xor(back, t) == 0 and back.block_table()[0].tolist() == kinds
                            assert bm.count_and(t, t) == cnt
                            u = bm.bvector._op2(bm.OR, t, x, bm.opt_none)
                            eu = port.op2(bm.OR, port.op2(op, pa, pb, opt), pa, False)
                            assert (u.to_words(nw) == eu.to_words(nw)).all() and u.block_table()[0].tolist() == eu.flatten()[0].tolist()
                            del back, u
                        del t
    finally:
        ctx.set_tuning("op2_loop", -1); ctx.set_tuning("op2_nt", 3)


@pytest.mark.parametrize("nblk", [3, 2300])
def test_async_pairwise_chain(ctx, port, nblk):
    """bmx_op2_dev / bmx_pending_wait: chains of three-operand operations that stay on the stream (operands = vectors without
    GAP blocks or unresolved results) give the oracle's bits AND block kinds after one wait at the end -- the streaming kernel
    (two all-bit-block vectors), the persistent and the wave-per-column kernels (operands with NULL / FULL blocks, unresolved
    operands, different lengths), results that come out empty or sparse (compacted at the wait), an operand used twice,
    waiting out of order, dropping an unresolved result; chains over operands WITH GAP blocks (results with GAP blocks as operands)"""
    rng = np.random.default_rng(nblk)
    def build(seed, dq, nb, holes):
        w = port.gen_words(777, seed, dq, nb * 65536)
        for b in rng.choice(nb, size=holes, replace=False):
            w[b * 2048:(b + 1) * 2048] = 0 if b % 2 else 0xFFFFFFFF
        return w
    ws = [build(1, 20000, nblk, 0), build(2, 30000, nblk, 0), build(3, 25000, nblk, max(1, nblk // 5)), build(4, 32768, max(1, nblk - 1), max(1, nblk // 3))]
    pv = [port.import_words(w, False, w.size * 32) if i < 2 else port.import_words(w, True, w.size * 32) for i, w in enumerate(ws)]
    gv = [bm.bit_import_u32(ctx, w, False) if i < 2 else bm.bit_import_u32(ctx, w, True) for i, w in enumerate(ws)]
    assert all(v.calc_stat()["gap_blocks"] == 0 for v in gv)
    nw = nblk * 2048
    def same(t, e):
        return (t.to_words(nw) == e.to_words(nw)).all() and t.block_table()[0].tolist() == (e.flatten()[0].tolist() + [0] * nblk)[:t.info()["nblocks"]] and t.count() == e.count()
    # a chain: r1 = v0 & v1 (streaming kernel); r2 = r1 | v2 (unresolved operand); r3 = r2 - v3; r4 = r3 ^ r1; r5 = r4 & r4
    r1 = bm.bvector.op2_async(bm.AND, gv[0], gv[1])
    r2 = bm.bvector.op2_async(bm.OR, r1, gv[2])
    r3 = bm.bvector.op2_async(bm.SUB, r2, gv[3])
    r4 = bm.bvector.op2_async(bm.XOR, r3, r1)
    r5 = bm.bvector.op2_async(bm.AND, r4, r4)
    r6 = bm.bvector.op2_async(bm.XOR, r4, r4)                                   # empty
    r7 = bm.bvector.op2_async(bm.AND, gv[2], gv[3])                             # sparse-ish: NULL / FULL holes on both sides
    e1 = port.op2(bm.AND, pv[0], pv[1], False); e2 = port.op2(bm.OR, e1, pv[2], False); e3 = port.op2(bm.SUB, e2, pv[3], False)
    e4 = port.op2(bm.XOR, e3, e1, False); e5 = port.op2(bm.AND, e4, e4, False); e6 = port.op2(bm.XOR, e4, e4, False)
    e7 = port.op2(bm.AND, pv[2], pv[3], False)
    t5 = r5.wait()                                                              # out of order: the last link first
    assert same(t5, e5)
    t7, t6, t4, t3, t2, t1 = r7.wait(), r6.wait(), r4.wait(), r3.wait(), r2.wait(), r1.wait()
    for t, e in ((t1, e1), (t2, e2), (t3, e3), (t4, e4), (t6, e6), (t7, e7)):
        assert same(t, e)
    assert t6.count() == 0
    # resolved results are ordinary vectors: operands of the synchronous entries, downloadable
    u = bm.bvector.bit_or(t3, t7)
    assert same(u, port.op2(bm.OR, e3, e7, False))
    k, o, b, g = t7.block_table()
    assert bm.count_xor(bm.bvector.from_block_table(ctx, t7.info()["nbits"], k, o, b, g), t7) == 0
    # dropping an unresolved result that later operations read; GAP operands are refused
    d1 = bm.bvector.op2_async(bm.OR, gv[0], gv[2]); d2 = bm.bvector.op2_async(bm.AND, d1, gv[1]); del d1
    assert same(d2.wait(), port.op2(bm.AND, port.op2(bm.OR, pv[0], pv[2], False), pv[1], False))
    # operands WITH GAP blocks (sparse, mixed 1 %, long runs): the results hold GAP blocks too -- laid out by the kernel, converted
    # right behind it, usable as operands at once; kinds and bits = the oracle's for every link
    mw = [port.gen_words(777, 20, 13, nblk * 65536), port.gen_words(777, 21, 655, nblk * 65536), port.gen_words(777, 22, 300, nblk * 65536)]
    mw[2][100:700] = 0xFFFFFFFF
    mp = [port.import_words(w, True, w.size * 32) for w in mw]
    mg = [bm.bit_import_u32(ctx, w, True) for w in mw]
    assert sum(v.calc_stat()["gap_blocks"] for v in mg) > 0
    q1 = bm.bvector.op2_async(bm.OR, mg[0], mg[2])                             # GAP | GAP
    q2 = bm.bvector.op2_async(bm.AND, q1, mg[1])                               # unresolved (GAP candidates) & mixed
    q3 = bm.bvector.op2_async(bm.SUB, mg[1], q2)
    q4 = bm.bvector.op2_async(bm.XOR, q3, gv[0])                               # ... against a dense vector
    q5 = bm.bvector.op2_async(bm.AND, mg[0], mg[0])                            # a vector with itself: a copy, GAP blocks stay GAP
    f1 = port.op2(bm.OR, mp[0], mp[2], False); f2 = port.op2(bm.AND, f1, mp[1], False); f3 = port.op2(bm.SUB, mp[1], f2, False)
    f4 = port.op2(bm.XOR, f3, pv[0], False); f5 = port.op2(bm.AND, mp[0], mp[0], False)
    u4 = q4.wait(); u5 = q5.wait(); u1 = q1.wait(); u3 = q3.wait(); u2 = q2.wait()
    for t, e in ((u1, f1), (u2, f2), (u3, f3), (u4, f4), (u5, f5)):
        assert same(t, e)
    k, o, b, g = u2.block_table()                                               # GAP data in arrival order, trimmed slab: a plain host table
    assert bm.count_xor(bm.bvector.from_block_table(ctx, u2.info()["nbits"], k, o, b, g), u2) == 0
    assert same(bm.bvector.bit_or(u1, u3), port.op2(bm.OR, f1, f3, False))


def test_pairwise_gap_results_converted_by_the_kernel(ctx):
    """Round 5: k_op2_loop converts its own GAP results in a tail phase (workgroup list of up to 80 candidates, dealt round the
    waves; a workgroup with more finds them again through st[] / gap_offs[]).  Two sparse 1.7e9-bit vectors, every block a GAP
    block, so EVERY result block of OR / XOR / SUB / AND is a GAP block: at one workgroup per CU (op2_loop 1) a workgroup parks
    ~100 candidates (the overflow path), at the default ~25 (the list), and the wave-per-column kernel with the layout scan and
    k_emit_gaps (op2_loop 0) is the older path: same bits, same block kinds, same counts as bm::count_*; the synchronous and
    the asynchronous entry; results as operands and as host block tables."""
    nbits = 1_700_000_000
    a = bm.bvector.generate(ctx, 0xABCD, 1, 20, nbits)
    b = bm.bvector.generate(ctx, 0xABCD, 2, 26, nbits)
    nblk = a.info()["nblocks"]
    assert a.calc_stat()["gap_blocks"] == nblk and b.calc_stat()["gap_blocks"] == nblk
    counts = {op: f(a, b) for op, f in ((bm.AND, bm.count_and), (bm.OR, bm.count_or), (bm.XOR, bm.count_xor), (bm.SUB, bm.count_sub))}
    try:
        ref = {}
        for loop in (0, -1, 1):
            ctx.set_tuning("op2_loop", loop)
            for op in (bm.OR, bm.XOR, bm.SUB, bm.AND):
                t = bm.bvector._op2(op, a, b, bm.opt_none)
                kinds = t.block_table()[0]
                assert t.count() == counts[op], (loop, op)
                if op != bm.AND: assert int((kinds == 3).sum()) == nblk, (loop, op)          # every block a GAP block
                if loop == 0: ref[op] = (t, kinds)
                else:
                    assert bm.count_xor(t, ref[op][0]) == 0 and (kinds == ref[op][1]).all(), (loop, op)
                    k, o, bb, g = t.block_table()
                    back = bm.bvector.from_block_table(ctx, nbits, k, o, bb, g)
                    assert bm.count_xor(back, ref[op][0]) == 0
                    assert bm.count_and(t, a) == {bm.AND: counts[bm.AND], bm.SUB: counts[bm.SUB], bm.XOR: counts[bm.SUB], bm.OR: a.count()}[op]
                    if loop == 1:
                        u = bm.bvector.op2_async(op, a, b).wait()
                        assert bm.count_xor(u, ref[op][0]) == 0 and (u.block_table()[0] == ref[op][1]).all()
    finally:
        ctx.set_tuning("op2_loop", -1)


def test_full_size_pairwise_and_rank_select_vs_reference_on_all_cores(ctx):
    """BASELINE configs[1] and configs[3] at FULL size against the reference itself (oracle/_ref, the unmodified BitMagic;
    the C port where it is absent) fanned over the host cores by block range -- not only identities: the four counts of a
    whole 2 x 1e9-bit pair, and the total + sampled rank / select answers over a 4e9-bit vector (per-range indexes, totals
    prefix-summed: the one exchange SURVEY 8(e) names)"""
    import os, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if root not in sys.path: sys.path.insert(0, root)
    import bench
    cores = min(len(os.sched_getaffinity(0)), 128)
    nbits = 1_000_000_000
    for dq in (6554, 655):
        a = bm.bvector.generate(ctx, bench.SEED, 1, dq, nbits); b = bm.bvector.generate(ctx, bench.SEED, 2, dq, nbits)
        ref = bench.cpu_pair_allcores(1, 2, dq, nbits, cores, reps=1)
        assert [bm._count_op2(op, a, b) for op in range(4)] == ref["full_counts"], dq
        del a, b
    nb4 = 4_000_000_000
    rng = np.random.default_rng(5)
    for dq in (6554, 655):
        v = bm.bvector.generate(ctx, bench.SEED, 7, dq, nb4)
        rs = v.build_rs_index()
        sn = rng.integers(0, nb4, 5000, dtype=np.uint64)
        total, sn, an, sr, ar = bench.cpu_rank_allcores(7, dq, nb4, cores, sn, lambda tot: rng.integers(1, tot + 1, 5000, dtype=np.uint64))
        assert rs.count() == total == v.count()
        assert (v.count_to(sn, rs) == an).all()
        f, p = v.select(sr, rs)
        assert f.all() and (p == ar).all()
        del rs, v


def test_pairwise_on_uploaded_only_operands_fresh_context(port):
    """bmx_op2's laid-out path (k_op2_loop + bump cursor) writes a GAP candidate list behind offs[] in the
    context's scratch.  On a FRESH context whose only vectors came through bmx_vec_upload (the C++ facade's path: nothing has
    grown the scratch before) >= 2,048 all-GAP blocks per operand must not overrun it: results = the oracle, and vectors that
    were allocated right before the call keep their bits."""
    c = bm.context(0)
    try:
        nblk = 4100
        wa = port.gen_words(9100, 1, 120, nblk * 65536); wb = port.gen_words(9100, 2, 120, nblk * 65536)
        pa, pb = port.import_words(wa, True, wa.size * 32), port.import_words(wb, True, wb.size * 32)
        ga = bm.bvector.from_block_table(c, wa.size * 32, *pa.flatten())
        gb = bm.bvector.from_block_table(c, wb.size * 32, *pb.flatten())
        assert ga.info()["counts"][bm.GAP] == nblk and gb.info()["counts"][bm.GAP] == nblk
        guard = bm.bvector.from_block_table(c, wa.size * 32, *pa.flatten())      # a neighbour in device memory
        for op in (bm.AND, bm.SUB, bm.OR, bm.XOR):
            t = bm.bvector._op2(op, ga, gb, bm.opt_none)
            e = port.op2(op, pa, pb, 0)
            assert t.block_table()[0].tolist() == e.flatten()[0].tolist(), op
            assert (t.to_words(wa.size) == e.to_words(wa.size)).all(), op
            del t
        assert bm.count_xor(guard, ga) == 0 and (guard.to_words(wa.size) == wa).all()
    finally:
        c.close()


@pytest.mark.parametrize("nvec,nsub", [(40, 0), (70, 9), (300, 33)])
def test_and_rows_kernel(ctx, port, nvec, nsub):
    """Round 5: AND / AND-SUB over GAP-only operands straight from the operands' slabs (k_agg_and_rows, bmx_kernels9.h: union of
    the AND operands' 0-runs, complemented, minus the union of the SUB operands' 1-runs), counts pipelines (several groups,
    block-range runs) and the materialising combine_and_sub: counts, bits and block kinds = the oracle and = the older
    kernels, for every launch shape.  Blocks of one, two and three 1-KiB pieces (up to 1,201 runs), blocks that start with a
    1-run, inverted (dense) GAP blocks, single-run blocks, FULL / NULL operands, ragged operand lengths, more than 64 operands
    per wave (two entry batches), SUB lists longer than the AND list."""
    nblk = 6
    nbits = nblk * 65536 - 4321
    nw = nblk * 2048
    rng = np.random.default_rng(nvec * 17 + nsub)
    common = port.gen_words(777, 0xFFFFFFFF, 40, nblk * 65536)
    common[5] |= 1                                                     # bit 0 of the vector survives in every AND operand
    words = []
    for v in range(nvec + nsub):
        nb_v = nbits if v % 7 else nbits - 2 * 65536                   # ragged: some operands end two blocks early
        w = port.gen_words(777, v, (30, 120, 300)[v % 3], nblk * 65536)
        for b in range(nblk):
            lo, r = b * 2048, rng.integers(0, 16)
            if r == 0 and v >= nvec: w[lo:lo + 2048] = 0                                       # NULL block (SUB operand)
            elif r == 1: w[lo:lo + 2048] = 0xFFFFFFFF                                          # FULL block
            elif r == 2: w[lo:lo + 2048] = ~w[lo:lo + 2048]                                    # dense GAP: long 1-runs, starts with a 1-run
            elif r == 3:                                                                       # 560 isolated bits: 1,121 runs (+ the shared ones), three pieces
                w[lo:lo + 2048] = 0
                pos = np.arange(560) * 116 + 1 + (v % 50)
                np.bitwise_or.at(w, lo + (pos >> 5), (np.uint32(1) << (pos & 31).astype(np.uint32)))
            elif r == 4: w[lo] |= 1                                                            # starts with a 1-run
            elif r == 5 and v < nvec: w[lo:lo + 2048] = 0xFFFFFFFF; w[lo + 2047] = 0x7FFFFFFF  # two runs: all ones but the last bit
        if v < nvec: w |= common                                        # the AND survives (also in the inverted and the 600-bit blocks)
        nwv = (nb_v + 31) // 32
        if nb_v % 32: w[nwv - 1] &= np.uint32((1 << (nb_v % 32)) - 1)
        w[nwv:] = 0
        words.append(w)
    lens = [nbits if v % 7 else nbits - 2 * 65536 for v in range(nvec + nsub)]
    gv = [bm.bit_import_u32(ctx, w[:(n + 31) // 32], True) for w, n in zip(words, lens)]
    pv = [port.import_words(w[:(n + 31) // 32], True, n) for w, n in zip(words, lens)]
    assert all(v.calc_stat()["bit_blocks"] == 0 for v in gv), "the case must stay GAP-only"
    A, S = list(range(nvec)), list(range(nvec, nvec + nsub))
    groups = [(A, S), (A[::2], []), (A[:nvec // 2], S[:1]), (A[:17], S), (A[3:4] * 1 + A[5:21], [])]
    exp = port.pipeline_counts([([pv[i] for i in a], [pv[i] for i in s]) for a, s in groups])
    pipe = bm.aggregator.pipeline(ctx)
    for a, s in groups:
        ag = pipe.add()
        for i in a: ag.add(gv[i], 0)
        for i in s: ag.add(gv[i], 1)
    pipe.complete()
    agg = bm.aggregator(ctx)
    try:
        ctx.set_tuning("pipe_split", 0); ctx.set_tuning("direct_cols", 0)     # (so few items / columns would take the one-workgroup-per-item kernels)
        for ar, wg, depth, nt in ((1, 256, 2, 0), (1, 512, 4, 1), (1, 512, 8, 0), (1, 256, 8, 1), (1, 128, 3, 0), (0, 512, 4, 0), (-1, 256, 3, 0)):
            ctx.set_tuning("and_rows", ar); ctx.set_tuning("and_rows_wg", wg); ctx.set_tuning("and_rows_depth", depth); ctx.set_tuning("and_rows_nt", nt)
            ctx.set_tuning("and_rows_ipw", (1, 3, 8)[depth % 3])                  # (items per workgroup: several groups of a column share one)
            d = pipe.describe()
            assert ("k_agg_and_rows<COUNT,%d,%d>" % (wg, depth) in d) == (ar != 0), d
            got = agg.combine_and_sub(pipe)
            assert (got == exp).all(), (ar, wg, depth, nt, got, exp)
            parts = sum(agg._run_pipeline(pipe, a, b).astype(np.int64) for a, b in [(0, 1), (1, 4), (4, nblk)])
            assert (parts == exp.astype(np.int64)).all(), (ar, wg, depth)
            for a, s in groups[:4]:
                e = port.agg_and_sub([pv[i] for i in a], [pv[i] for i in s])
                t, any_ = agg.combine_and_sub([gv[i] for i in a], [gv[i] for i in s])
                assert (t.to_words(nw) == e.to_words(nw)).all(), (ar, wg, depth, len(a), len(s))
                assert t.block_table()[0].tolist() == (e.flatten()[0].tolist() + [0] * nblk)[:t.info()["nblocks"]] and any_ == (e.count() != 0)
        # a results pipeline (one launch per group through agg_and_sub_launch) with the row kernel forced
        ctx.set_tuning("and_rows", 1)
        rp = bm.aggregator.pipeline(ctx, bm.agg_opt_bvect_and_counts)
        for a, s in groups:
            ag = rp.add()
            for i in a: ag.add(gv[i], 0)
            for i in s: ag.add(gv[i], 1)
        rp.complete()
        res = agg.combine_and_sub(rp)
        for (a, s), r, c in zip(groups, res, rp.get_bv_count_vector()):
            e = port.agg_and_sub([pv[i] for i in a], [pv[i] for i in s])
            assert int(c) == e.count()
            assert (r is None) == (e.count() == 0)
            if r is not None: assert (r.to_words(nw) == e.to_words(nw)).all()
    finally:
        for k, v in (("and_rows", -1), ("and_rows_wg", 256), ("and_rows_depth", 3), ("and_rows_nt", 0), ("and_rows_ipw", 0), ("pipe_split", -1), ("direct_cols", 384)):
            ctx.set_tuning(k, v)


def test_search_count_limit_drops_groups_per_group(ctx, port):
    """pipeline::set_search_count_limit per ARG-GROUP (src/bmaggregator.h:1362-1367: a group at its limit is skipped on every
    following block).  1,000 groups of which ONE has fewer hits than the limit: the first launch window runs over all of them,
    every later window over that one group only (bmx_pipeline_last_window_groups); the satisfied groups return >= limit and
    <= their true count, the short one its true count.  Same through the LDS-staged kernel and over GAP-only operands
    (k_agg_and_rows).  Results + counts runs truncate a group's vector at the window where it had enough; result-only runs
    ignore the limit; bm::id_max means no limit."""
    ncols = 2000
    nbits = ncols * 65536
    dense = [bm.bvector.generate(ctx, SEED, 700 + i, 6554, nbits, with_common=True) for i in range(8)]
    sparse = bm.bvector.generate(ctx, SEED, 790, 2, nbits)                 # ~2 bits per block
    agg = bm.aggregator(ctx)
    pairs = [(i, j) for i in range(8) for j in range(8) if i != j]
    def mk(ngroups, limit, opt=bm.agg_opt_only_counts, short_at=None):
        pipe = bm.aggregator.pipeline(ctx, opt)
        for g in range(ngroups):
            ag = pipe.add()
            if g == short_at:
                ag.add(dense[0], 0); ag.add(sparse, 0)
            else:
                i, j = pairs[g % len(pairs)]
                ag.add(dense[i], 0); ag.add(dense[j], 0)
                if g % 3 == 0: ag.add(dense[(i + j) % 8], 1 if (i + j) % 8 not in (i, j) else 0)
        if limit is not None: pipe.set_search_count_limit(limit)
        pipe.complete()
        return pipe
    ng, short = 1000, 617
    full = [int(x) for x in agg.combine_and_sub(mk(ng, None, short_at=short))]
    limit = 5000
    assert full[short] < limit and min(c for g, c in enumerate(full) if g != short) > 100 * limit
    try:
        for staged in (-1, 0):
            ctx.set_tuning("pipe_staged", staged)
            p = mk(ng, limit, short_at=short)
            got = [int(x) for x in agg.combine_and_sub(p)]
            launched, planned = p.last_windows()
            wg = p.last_window_groups()
            assert launched == planned == len(wg) and planned >= 3, (staged, launched, planned, wg)
            assert wg[0] == ng and all(x == 1 for x in wg[1:]), (staged, wg)
            assert got[short] == full[short]
            assert all(limit <= g <= t for k, (g, t) in enumerate(zip(got, full)) if k != short), staged
            # the satisfied groups stopped after the first window: they hold what that window found, far below their true count
            assert all(g < t // 8 for k, (g, t) in enumerate(zip(got, full)) if k != short)
            # round 6: the ASYNCHRONOUS entry honours the limit too -- every window enqueued over all groups, a finished group
            # pointed at null table entries on the device (k_limit_null): same windows, same totals, no host decision in between
            dev = _dev_counts(ctx, agg, p, ng)
            assert dev == got, (staged, [(k, a, b) for k, (a, b) in enumerate(zip(dev, got)) if a != b][:5])
    finally:
        ctx.set_tuning("pipe_staged", -1)
    # every group satisfied in the first window: nothing else is launched
    p = mk(64, limit); got = agg.combine_and_sub(p)
    assert p.last_windows()[0] == 1 and p.last_window_groups() == [64] and all(int(g) >= limit for g in got)
    # bm::id_max = no limit: one plain run
    p = mk(64, None); p.set_search_count_limit(bm.ID_MAX)
    assert [int(x) for x in agg.combine_and_sub(p)] == full[:64]
    assert p.last_windows() == (1, 1)
    # results + counts: a group's vector ends where its count passed the limit; result-only runs ignore the limit
    pr = mk(40, limit, opt=bm.agg_opt_bvect_and_counts, short_at=7)
    res = agg.combine_and_sub(pr)
    cnt = [int(x) for x in pr.get_bv_count_vector()]
    pf = mk(40, None, opt=bm.agg_opt_bvect_and_counts, short_at=7)
    res_full = agg.combine_and_sub(pf)
    cnt_full = [int(x) for x in pf.get_bv_count_vector()]
    for g in range(40):
        assert cnt[g] == res[g].count() and min(limit, cnt_full[g]) <= cnt[g] <= cnt_full[g], g
        assert bm.count_and(res[g], res_full[g]) == cnt[g]                     # a subset of the unlimited result ...
        if g != 7:
            assert cnt[g] < cnt_full[g] // 8
            last = int(res[g].to_indices()[-1]) >> 16                           # ... namely its leading block columns
            assert bm.count_and(res[g], res_full[g]) == res_full[g].count_range(0, (last + 1) * 65536 - 1, res_full[g].build_rs_index())
        else:
            assert cnt[g] == cnt_full[g]
    po = mk(12, limit, opt=bm.agg_run_options(True, False))                    # results only: the limit does not apply (:1362 is under is_compute_counts)
    ro = agg.combine_and_sub(po)
    assert [r.count() for r in ro] == [int(x) for x in agg.combine_and_sub(mk(12, None))]
    # GAP-only operands (k_agg_and_rows) under a limit
    gaps = [bm.bvector.generate(ctx, SEED, 900 + i, 120, nbits, with_common=True) for i in range(24)]
    def mkg(limit):
        pipe = bm.aggregator.pipeline(ctx)
        for g in range(6):
            ag = pipe.add()
            for v in (gaps[g * 4:(g + 1) * 4] * 3 if g != 2 else gaps[8:12] * 2 + [sparse]): ag.add(v, 0)
        if limit: pipe.set_search_count_limit(limit)
        pipe.complete()
        return pipe
    pg = mkg(None)
    assert "k_agg_and_rows" in pg.describe()
    fg = [int(x) for x in agg.combine_and_sub(pg)]
    lim = max(fg[2] + 1, 50)
    pg2 = mkg(lim); gg = [int(x) for x in agg.combine_and_sub(pg2)]
    wgs = pg2.last_window_groups()
    assert gg[2] == fg[2] and all(min(lim, t) <= g <= t for g, t in zip(gg, fg)) and wgs[0] == 6 and wgs[-1] == 1, (gg, fg, wgs)
    assert _dev_counts(ctx, agg, pg2, 6) == gg                                 # the asynchronous entry over GAP-only operands
    assert _dev_counts(ctx, agg, pg, 6) == fg                                  # ... and without a limit
    # ... and over the members of a packed collection (k_coll_members: a finished group gets an empty member range)
    ctx.collection_prepare(gaps, bm.ROLE_AND)
    try:
        ctx.set_tuning("coll_members", 1)
        pg3 = mkg(lim); g3 = [int(x) for x in agg.combine_and_sub(pg3)]
        assert g3[2] == fg[2] and all(min(lim, t) <= g <= t for g, t in zip(g3, fg)), (g3, fg)
        assert _dev_counts(ctx, agg, pg3, 6) == g3
    finally:
        ctx.set_tuning("coll_members", -1)


def _dev_counts(ctx, agg, pipe, ng):
    import torch
    d = torch.full((ng,), -1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    agg.run_counts_dev(pipe, d.data_ptr())
    ctx.synchronize()
    return [int(x) for x in d.cpu().tolist()]


def test_many_unresolved_asynchronous_results(ctx, port):
    """bmx_op2_dev: up to 1,024 results may be outstanding per context (round 6; 64 before: VERDICT r5 weak #8).  300 operations enqueued
    without a wait, resolved afterwards in reverse order: every count = the oracle's; the 1,025th unresolved result is BMX_ERR_RANGE and
    the context goes on after the others are resolved"""
    nbits = 6 * 65536 - 17
    ws = [port.gen_words(SEED, 50 + i, 6554 if i % 2 else 655, nbits) for i in range(6)]
    pv = [port.import_words(w, True, nbits) for w in ws]
    gv = [bm.bvector.from_block_table(ctx, nbits, *p.flatten()) for p in pv]
    exp = {(op, i, j): port.op2(op, pv[i], pv[j]).count() for op in (bm.AND, bm.OR, bm.XOR, bm.SUB) for i in range(6) for j in range(6) if i != j}
    keys = list(exp)[:100] * 3
    pend = [bm.bvector.op2_async(op, gv[i], gv[j]) for op, i, j in keys]
    for k, p in reversed(list(zip(keys, pend))):
        assert p.wait().count() == exp[k], k
    pend = [bm.bvector.op2_async(bm.AND, gv[0], gv[1]) for _ in range(1024)]
    with pytest.raises(bm.BmxError) as e:
        bm.bvector.op2_async(bm.AND, gv[0], gv[1])
    assert e.value.status == 3
    for p in pend[:5]: assert p.wait().count() == exp[(bm.AND, 0, 1)]
    del pend
    assert bm.bvector.op2_async(bm.OR, gv[2], gv[3]).wait().count() == exp[(bm.OR, 2, 3)]


def test_op2_count_in_one_call(ctx, port):
    """bmx_op2_count (result + count from one call): for short vectors the pairwise kernel folds the popcount of
    its result, so bit_and + count() is one launch (the count travels with the vector: bmx_count after bmx_op2 launches
    nothing); long vectors, GAP operands, opt_compress, empty and full results, count-only form = the oracle"""
    rng = np.random.default_rng(77)
    for nbits, dqa, dqb in ((1_000_000, 6554, 6554), (40 * 65536 + 17, 655, 300), (2100 * 65536, 6554, 655), (3 * 65536, 65536, 40)):
        wa, wb = port.gen_words(SEED, 11, dqa, nbits), port.gen_words(SEED, 12, dqb, nbits)
        pa, pb = port.import_words(wa, True, nbits), port.import_words(wb, True, nbits)
        ga, gb = bm.bvector.from_block_table(ctx, nbits, *pa.flatten()), bm.bvector.from_block_table(ctx, nbits, *pb.flatten())
        for op in (bm.AND, bm.OR, bm.XOR, bm.SUB):
            for opt in (bm.opt_none, bm.opt_compress):
                e = port.op2(op, pa, pb, int(opt == bm.opt_compress))
                t, c = bm.bvector.op2_count(op, ga, gb, opt)
                assert c == e.count() and t.count() == c, (nbits, op, opt)
                assert t.block_table()[0].tolist() == e.flatten()[0].tolist()
                t2 = bm.bvector._op2(op, ga, gb, opt)
                assert t2.count() == c
            none, c = bm.bvector.op2_count(op, ga, gb, want_result=False)
            assert none is None and c == port.count_op2(op, pa, pb)


@pytest.mark.parametrize("dq,nvec,nblk,long_runs", [(13, 70, 30, False), (13, 333, 17, True), (40, 129, 45, True), (150, 64, 9, False), (5, 1100, 15, False)])
def test_collection_tile_build_equals_column_build(port, dq, nvec, nblk, long_runs):
    """Round 5: bmx_collection_prepare(ROLE_OR) through the tile directories (k_coll2_count / k_coll2_scatter, bmx_kernels10.h:
    coll_build 1) builds the collection the (operand, column tile) passes of rounds 3 / 4 build (coll_build 0): the full union
    (k_coll_apply streams the column regions), random subsets and SUB lists forced through the member directory
    (k_coll_members reads dir / dir_s), a counts pipeline over it -- all equal to the oracle's bits, block kinds and counts
    under both builds.  Rows the directory cannot describe (FULL blocks, blocks starting with a 1-run, tiles of more than 64
    chunks: long_runs / specials), NULL-only operands, operands of different lengths, operand counts that are no multiple
    of 64, more than 1,024 operands (17 groups)."""
    rng = np.random.default_rng(dq * 131 + nvec)
    nbits = nblk * 65536 - 777
    words = _sparse_collection(port, rng, nvec, nbits, dq, long_runs=long_runs, ragged=True, specials=True)
    for v in range(0, nvec, 9):                                            # blocks that start with a 1-run; an all-NULL operand
        b = int(rng.integers(0, nblk))
        if (b + 1) * 2048 <= words[v].size: words[v][b * 2048] |= np.uint32(1)
    words[min(7, nvec - 1)][:] = 0
    pv = [port.import_words(w, True, w.size * 32) for w in words]
    assert all(p.flatten()[0].tolist().count(2) == 0 for p in pv), "operands must be free of bit-blocks"
    nwb = (nblk + 1) * 2048
    subsets = [rng.choice(nvec, size=int(rng.integers(16, nvec)), replace=False).tolist() for _ in range(6)]
    e_all = port.agg_or(pv, False)
    stats = {}
    for build in (1, 0):
        c = bm.context(0)
        c.set_tuning("direct_cols", 0); c.set_tuning("pipe_split", 0); c.set_tuning("coll_build", build)
        gv = [bm.bvector.from_block_table(c, w.size * 32, *p.flatten()) if i % 3 else bm.bit_import_u32(c, w, True) for i, (w, p) in enumerate(zip(words, pv))]
        c.collection_prepare(gv, bm.ROLE_OR)
        st = c.pack_stats(); assert st["collections"] == 1
        stats[build] = st["run_bytes"]                                        # (the tile build leaves the member directory to the first call that needs it)
        agg = bm.aggregator(c)
        o = agg.combine_or(gv)                                               # every member: the column regions as streams
        assert (o.to_words(nwb) == e_all.to_words(nwb)).all(), build
        assert o.block_table()[0].tolist() == (e_all.flatten()[0].tolist() + [0] * 8)[:o.info()["nblocks"]], build
        c.set_tuning("coll_members", 1); c.set_tuning("or_rows", 0)          # subsets: the members' pieces through the directory
        for k, sel in enumerate(subsets):
            o = agg.combine_or([gv[i] for i in sel])
            e = port.agg_or([pv[i] for i in sel], False)
            assert (o.to_words(nwb) == e.to_words(nwb)).all(), (build, k)
            assert o.block_table()[0].tolist() == (e.flatten()[0].tolist() + [0] * 8)[:o.info()["nblocks"]], (build, k)
        assert c.pack_stats()["collections"] == 1
        c.close()
    assert stats[0] == stats[1], stats                                        # same run bytes
