"""GPU: the OR side of the aggregator and the packed collections at every border of their kernels, on constructed cases
(tests/golden/or_cases.py: grids O1 .. O6; tests/test_or_host.py keeps the generator and its model honest on the CPU).
Every comparison is bit-exact -- the words of all 31 blocks, block kinds, count(), any -- against the closed form (the NumPy
union) and against the oracle port; recorded cases also against the reference's fixture (tests/golden/or_ref.json).
  O1, O2   every list through every OR path that takes GAP-only lists, each forced by its tuning keys, with the preconditions
           the host selection reads asserted (a list call has no describe()); the results equal across paths, kind for kind
  O3 .. O5 prepared collections in both roles under both builders and both bag formats: the full list in every shape of
           k_coll_apply, with and without launch windows; subsets, member lists and pipelines through the member directory
  O6       a list made of what every writer of a GAP slab produces, through the row kernel, the column-tile kernel and prepared
           collections; expected = the OR of the operands' own to_words()
A failure names its case.  Every test restores every tuning key it touches; collections live in contexts of their own."""
import json
import os

import numpy as np
import pytest

import or_cases as oc
import pair_cases as pc
import bitmagic_amd as bm

pytestmark = pytest.mark.gpu

_PV, _GV = {}, {}
KNOBS = (("or_rows", -1), ("or_depth", 4), ("or_tile", 0), ("direct_cols", 384), ("pipe_split", -1), ("gap_pack", -1),
         ("coll_members", -1), ("coll_shape", 4), ("coll_split", 1), ("coll_build", -1), ("coll_window", 0))
TABLES = (("direct_cols", 0), ("pipe_split", 0), ("gap_pack", 0))
# (name, tuning keys on top of TABLES, the operands of the list that are given)
PATHS = (("rows.d4", (("or_rows", 1), ("or_depth", 4)), None),
         ("rows.d8", (("or_rows", 1), ("or_depth", 8)), None),
         ("tile.0", (("or_rows", 0), ("or_tile", 0)), None),
         ("tile.1", (("or_rows", 0), ("or_tile", 1)), None),
         ("tile.2", (("or_rows", 0), ("or_tile", 2)), None),
         ("k_agg_or<2>", (("or_rows", 0),), 63),
         ("direct", (("direct_cols", 384), ("pipe_split", -1)), None))


@pytest.fixture(scope="module")
def octx():
    """a context of this module's own: no collection exists in it, ever"""
    c = bm.context(0)
    yield c
    _GV.clear()
    c.close()


@pytest.fixture(scope="module")
def fixture():
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "or_ref.json")) as f:
        return json.load(f)["cases"]


def restore(c):
    for key, x in KNOBS: c.set_tuning(key, x)


def kinds_of(v):
    return (v.block_table()[0].tolist() + [0] * oc.NBLOCKS)[:oc.NBLOCKS]


def port_kinds(e):
    return (e.flatten()[0].tolist() + [0] * oc.NBLOCKS)[:oc.NBLOCKS]


def popcount(w):
    return int(np.unpackbits(w.view(np.uint8)).sum())


def same(v, words, count, kinds, what):
    """words of all 31 blocks, block kinds, count(), any"""
    got = v.to_words(oc.NW)
    assert (got == words).all(), (what, "blocks that differ", np.unique(np.flatnonzero(got != words) // oc.BW))
    k = kinds_of(v)
    assert k == list(kinds), (what, "kinds", k, list(kinds))
    assert v.count() == count and v.any() == (count != 0), (what, "count", v.count(), count)


def preconditions(c, gv, path):
    """what bmx.hip's selection reads for the forced path: the list is long enough, holds GAP blocks and no bit-block, has
    columns, and no collection exists that could take it"""
    info = [g.info() for g in {id(g): g for g in gv}.values()]
    assert all(i["counts"][bm.BIT] == 0 for i in info) and any(i["counts"][bm.GAP] for i in info), path
    assert max(i["nblocks"] for i in info) > 0 and c.pack_stats()["collections"] == 0, path
    if path.startswith(("rows", "tile")): assert len(gv) >= oc.N_ROWS, path
    if path == "k_agg_or<2>": assert 0 < len(gv) < oc.N_ROWS, path
    if path == "direct": assert 24 <= len(gv) <= oc.DIRECT_MAX_OPS and max(i["nblocks"] for i in info) <= 384, path


@pytest.mark.parametrize("grid,k", oc.chunks())
def test_lists(octx, port, fixture, grid, k):
    """O1 / O2: aggregator.combine_or over every list of the chunk, through every path"""
    c = octx
    agg = bm.aggregator(c)
    try:
        for case in oc.chunk(grid, k):
            gv = [oc.device_vec(bm, c, o, _GV) for o in case.ops]
            pv = [oc.port_vec(port, o, _PV) for o in case.ops]
            w, cnt, k0, k1 = case.expect()
            w63 = case.expect(case.ops[:63])
            rec = fixture.get("%s/%s" % (grid, case.name))
            seen = {}
            for opt in (False, True):
                agg.set_optimization(opt)
                e = port.agg_or(pv, opt)
                assert (e.to_words(oc.NW) == w).all() and port_kinds(e) == (k1 if opt else k0), (case, opt)
                if rec:
                    r = rec["compress" if opt else "none"]
                    assert (r["kinds"], r["count"], r["sha"]) == (oc.kinds_str(k1 if opt else k0), cnt, oc.sha(w)), (case, opt)
                for path, knobs, first in PATHS:
                    if path == "direct" and len(gv) > oc.DIRECT_MAX_OPS: continue
                    restore(c)
                    for key, x in TABLES + knobs: c.set_tuning(key, x)
                    some = gv if first is None else gv[:first]
                    preconditions(c, some, path)
                    o = agg.combine_or(some)
                    if first is None:
                        same(o, w, cnt, k1 if opt else k0, (case, path, opt))
                        seen[path, opt] = kinds_of(o)
                    else:
                        same(o, w63[0], w63[1], w63[3] if opt else w63[2], (case, path, opt))
                        e63 = port.agg_or(pv[:first], opt)
                        assert (e63.to_words(oc.NW) == w63[0]).all() and port_kinds(e63) == kinds_of(o), (case, path, opt)
            assert len({tuple(v) for (p, opt), v in seen.items() if not opt}) == 1 and len({tuple(v) for (p, opt), v in seen.items() if opt}) == 1, case
    finally:
        agg.set_optimization(False)
        restore(c)


# ---------------------------------------------------------------------------------------------------------------------
# O3 .. O5: collections
# ---------------------------------------------------------------------------------------------------------------------
class Prepared:
    """a context of its own with the collection's vectors in both roles, prepared under one builder and one bag format"""

    def __init__(self, names, build, split, roles=("or", "and")):
        self.c = c = bm.context(0)
        for key, x in (("direct_cols", 0), ("pipe_split", 0), ("coll_build", build), ("coll_split", split)): c.set_tuning(key, x)
        self.gv, self.ncoll = {}, 0
        for name in names:
            for role in roles:
                vs = oc.coll(name).vecs(role)
                self.gv[name, role] = [bm.bvector.from_block_table(c, v.nbits, *v.block_table()) for v in vs]
                assert all(g.info()["counts"][bm.BIT] == 0 for g in self.gv[name, role])
                c.collection_prepare(self.gv[name, role], bm.ROLE_OR if role == "or" else bm.ROLE_AND)
                self.ncoll += 1
                assert c.pack_stats()["collections"] == self.ncoll, (name, role)

    def check(self):
        assert self.c.pack_stats()["collections"] == self.ncoll           # stays at what was prepared

    def close(self):
        for vs in self.gv.values(): vs.clear()
        self.c.close()


def and_words(C, idx=None):
    wa = C.words("and")
    return np.bitwise_and.reduce(wa if idx is None else wa[sorted(set(idx))], axis=0)


@pytest.mark.parametrize("build,split", [(0, 1), (1, 1), (0, 0), (1, 0)])
@pytest.mark.parametrize("name", oc.COLLS_FULL)
def test_collections_full_list(port, fixture, name, build, split):
    """O3 / O5: combine_or and combine_and_sub over ALL the vectors of a prepared collection (k_coll_apply in every shape, one
    launch and windows of five columns), a one-group counts pipeline in the AND role, subsets through the member directory"""
    C = oc.coll(name)
    u = C.union()
    inv = and_words(C)
    pv = [oc.port_vec(port, m, _PV) for m in C.members]
    pa = [oc.port_vec(port, m, _PV) for m in C.vecs("and")]
    e_or = {opt: port.agg_or(pv, opt) for opt in (False, True)}
    e_and, e_sub = port.agg_and_sub(pa, []), port.agg_and_sub(pa, pv)
    assert (e_and.to_words(oc.NW) == inv).all() and (e_sub.to_words(oc.NW) == inv).all()
    for opt in (False, True):
        kk = oc.kinds_of_union(u, C.members, opt)
        assert (e_or[opt].to_words(oc.NW) == u).all() and port_kinds(e_or[opt]) == kk
        r = fixture["coll/" + name]["compress" if opt else "none"]
        assert (r["kinds"], r["count"], r["sha"]) == (oc.kinds_str(kk), popcount(u), oc.sha(u)), (name, opt)
    P = Prepared([name], build, split)
    c, go, ga = P.c, P.gv[name, "or"], P.gv[name, "and"]
    agg = bm.aggregator(c)
    try:
        assert len(go) >= oc.N_MEMBERS
        for shape in range(6):
            for window in (0, 5):
                c.set_tuning("coll_shape", shape); c.set_tuning("coll_window", window)
                what = (name, build, split, shape, window)
                for opt in (False, True):
                    agg.set_optimization(opt)
                    same(agg.combine_or(go), u, popcount(u), port_kinds(e_or[opt]), what + ("or", opt))
                    same(agg.combine_or(go[::-1] + go[:3]), u, popcount(u), port_kinds(e_or[opt]), what + ("or, any order", opt))
                agg.set_optimization(False)
                t, any_ = agg.combine_and_sub(ga, [])
                same(t, inv, popcount(inv), port_kinds(e_and), what + ("and",))
                assert any_ == (popcount(inv) != 0)
                t, any_ = agg.combine_and_sub(ga, go)                      # the SUB bag: a FULL member empties its column
                same(t, inv, popcount(inv), port_kinds(e_sub), what + ("and-sub",))
                pipe = bm.aggregator.pipeline(c)
                ag = pipe.add()
                for x in ga: ag.add(x, 0)
                for x in go: ag.add(x, 1)
                pipe.complete()
                assert int(agg.combine_and_sub(pipe)[0]) == popcount(inv), what + (pipe.describe(),)
                assert "k_coll_apply<AND_COUNT" in pipe.describe(), pipe.describe()
                P.check()
        # subsets: the members' pieces through the directory
        c.set_tuning("coll_shape", 4); c.set_tuning("coll_window", 0); c.set_tuning("coll_members", 1)
        n = C.n
        for sel in (list(range(0, n, 2)), list(range(16)), list(range(n - 1, 0, -1)), list(range(n - 17, n)) + [0, 0, n - 1]):
            for opt in (False, True):
                agg.set_optimization(opt)
                e = port.agg_or([pv[i] for i in sel], opt)
                assert (e.to_words(oc.NW) == C.union(sel)).all()
                same(agg.combine_or([go[i] for i in sel]), C.union(sel), e.count(), port_kinds(e), (name, build, split, "subset or", sel[:4], opt))
            agg.set_optimization(False)
            e = port.agg_and_sub([pa[i] for i in sel], [pv[i] for i in sel[:5]])
            want = and_words(C, sel)                                       # (the SUB members lie inside the complement: nothing more goes)
            assert (e.to_words(oc.NW) == want).all()
            t, any_ = agg.combine_and_sub([ga[i] for i in sel], [go[i] for i in sel[:5]])
            same(t, want, popcount(want), port_kinds(e), (name, build, split, "subset and-sub", sel[:4]))
            P.check()
    finally:
        restore(c)
        del agg
        P.close()


def _pipelines(P, port, agg, C, S, pv, pa, ps, sub_name):
    """counts and results pipelines of 1, 3, 4 and 5 groups: AND lists from the AND-role collection, SUB lists from an OR-role one"""
    c = P.c
    w = C.words()
    ga, gs = P.gv["dir", "and"], P.gv[sub_name, "or"]
    for groups in oc.o4_pipelines():
        gl = [(a, [i % S.n for i in s]) for a, s in groups]
        sw = S.words()
        want_w = [and_words(C, a) & ~np.bitwise_or.reduce(sw[sorted(set(s))], axis=0) for a, s in gl]
        want = [popcount(x) for x in want_w]
        exp = port.pipeline_counts([([pa[i] for i in a], [ps[i] for i in s]) for a, s in gl])
        assert [int(x) for x in exp] == want
        for opts in (None, bm.agg_run_options(True, True)):
            pipe = bm.aggregator.pipeline(c) if opts is None else bm.aggregator.pipeline(c, opts)
            for a, s in gl:
                ag = pipe.add()
                for i in a: ag.add(ga[i], 0)
                for i in s: ag.add(gs[i], 1)
            pipe.complete()
            what = (sub_name, len(gl), "counts" if opts is None else "results")
            if opts is None:
                assert [int(x) for x in agg.combine_and_sub(pipe)] == want, what
                assert "k_coll_members" in pipe.describe(), pipe.describe()      # (the plan names the collections once a run resolved them)
            else:
                agg.combine_and_sub(pipe)
                assert [int(x) for x in pipe.get_bv_count_vector()] == want, what
                for g, r in enumerate(pipe.get_bv_res_vector()):
                    if want[g] == 0: assert r is None or r.count() == 0, what
                    else: assert (r.to_words(oc.NW) == want_w[g]).all() and r.count() == want[g], what + (g,)
            P.check()


@pytest.mark.parametrize("part", ["lists.0", "lists.1", "lists.2", "pipelines"])
@pytest.mark.parametrize("build", [0, 1])
def test_member_directory(port, build, part):
    """O4: member lists of 1 .. 129 members with the member under test (pieces of 0 .. 33 multi-bit and single-bit entries) at
    the borders of a step of four members and of a batch of 64; reversed lists, repeats; pipelines whose waves share a column"""
    C, S = oc.coll("dir"), oc.coll("short")
    pv = [oc.port_vec(port, m, _PV) for m in C.members]
    pa = [oc.port_vec(port, m, _PV) for m in C.vecs("and")]
    ps = [oc.port_vec(port, m, _PV) for m in S.members]
    P = Prepared(["dir"], build, 1)
    c = P.c
    P.gv["short", "or"] = [bm.bvector.from_block_table(c, v.nbits, *v.block_table()) for v in S.members]
    c.collection_prepare(P.gv["short", "or"], bm.ROLE_OR)
    P.ncoll += 1
    P.check()
    go, ga = P.gv["dir", "or"], P.gv["dir", "and"]
    agg = bm.aggregator(c)
    try:
        c.set_tuning("coll_members", 1)
        for m, p, t, order, l in (oc.o4_lists()[int(part[-1])::3] if part.startswith("lists") else ()):
            what = (build, m, p, t, order)
            for opt in (False, True):
                agg.set_optimization(opt)
                e = port.agg_or([pv[i] for i in l], opt)
                assert (e.to_words(oc.NW) == C.union(l)).all()
                same(agg.combine_or([go[i] for i in l]), C.union(l), e.count(), port_kinds(e), what + ("or", opt))
            agg.set_optimization(False)
            want = and_words(C, l)
            e = port.agg_and_sub([pa[i] for i in l], [])
            assert (e.to_words(oc.NW) == want).all()
            tt, any_ = agg.combine_and_sub([ga[i] for i in l], [])
            same(tt, want, popcount(want), port_kinds(e), what + ("and",))
            P.check()
        if part == "pipelines":
            _pipelines(P, port, agg, C, C, pv, pa, pv, "dir")
            _pipelines(P, port, agg, C, S, pv, pa, ps, "short")           # more columns than the SUB collection's vectors
    finally:
        restore(c)
        del agg
        P.close()


@pytest.mark.parametrize("build", [0, 1])
@pytest.mark.parametrize("name", oc.COLLS_DIR[1:])
def test_directory_sizes(port, name, build):
    """O4: collections of 31 .. 65 vectors (the 32 x 32 transposition tiles of k_coll_dir, entry n = the column's total): the full
    list, and lists that name the last member, all but one member, and members twice"""
    C = oc.coll(name)
    n = C.n
    pv = [oc.port_vec(port, m, _PV) for m in C.members]
    pa = [oc.port_vec(port, m, _PV) for m in C.vecs("and")]
    P = Prepared([name], build, 1)
    c, go, ga = P.c, P.gv[name, "or"], P.gv[name, "and"]
    agg = bm.aggregator(c)
    try:
        c.set_tuning("coll_members", 1)
        for sel in (list(range(n)), list(range(n - 1, 0, -1)), list(range(n - 16, n)), list(range(16)) + [n - 1, n - 1, 0]):
            for opt in (False, True):
                agg.set_optimization(opt)
                e = port.agg_or([pv[i] for i in sel], opt)
                assert (e.to_words(oc.NW) == C.union(sel)).all()
                same(agg.combine_or([go[i] for i in sel]), C.union(sel), e.count(), port_kinds(e), (name, build, "or", len(sel), opt))
            agg.set_optimization(False)
            want = and_words(C, sel)
            e = port.agg_and_sub([pa[i] for i in sel], [pv[i] for i in sel[:2]])
            assert (e.to_words(oc.NW) == want).all()
            t, any_ = agg.combine_and_sub([ga[i] for i in sel], [go[i] for i in sel[:2]])
            same(t, want, popcount(want), port_kinds(e), (name, build, "and-sub", len(sel)))
            P.check()
    finally:
        restore(c)
        del agg
        P.close()


# ---------------------------------------------------------------------------------------------------------------------
# O6: every writer of a GAP slab is a valid row operand
# ---------------------------------------------------------------------------------------------------------------------
BIT_BY_DESIGN = ("set", "keep")         # OR / AND with an index vector imported WITHOUT optimize: every touched block is a bit-block


def _producers(c, port):
    """(name, device vector) of what every writer of a GAP slab gives; where the producer can express arbitrary content it is
    asked for a pattern of or_cases.o6_pattern, and must give exactly that"""
    out = []
    agg = bm.aggregator(c)

    def pat(j):
        blocks, bits = oc.o6_pattern(j)
        return blocks, bits, oc.words_of(bits)

    def add(name, v, words=None):
        if words is not None: assert (v.to_words(oc.NW) == words).all(), name
        out.append((name, v))
        return v

    for j in range(4):
        blocks, bits, w = pat(j)
        wb = pat(j + 5)[2]
        ids = np.flatnonzero(bits)
        imp = add("bit_import_u32.%d" % j, bm.bit_import_u32(c, w, True), w)
        t = oc.Vec([None if not b.any() else "full" if b.all() else b for b in blocks])
        add("from_block_table.%d" % j, bm.bvector.from_block_table(c, t.nbits, *t.block_table()), w)
        add("generate.%d" % j, bm.bvector.generate(c, 4242, j, 13, oc.NBITS, optimize=True))
        add("from_indices.%d" % j, bm.bvector.from_indices(c, ids.astype(np.uint32), oc.NBITS, optimize=True), w)
        add("from_indices.u64.unsorted.%d" % j, bm.bvector.from_indices(c, ids[::-1].astype(np.uint64), oc.NBITS, optimize=True), w)
        add("from_ranges.%d" % j, bm.bvector.from_ranges(c, oc.ranges_of(bits), oc.NBITS), w)
        # set / keep / clear: this OP an index vector of bit-blocks.  clear() of every bit of two columns leaves NULL blocks there
        # and copies of the GAP blocks everywhere else
        base = lambda: bm.bvector.from_indices(c, ids.astype(np.uint32), oc.NBITS, optimize=True)
        two = ids[(ids >> 16 == 3) | (ids >> 16 == 20)].astype(np.uint32)
        w2 = w.copy(); w2[3 * oc.BW:4 * oc.BW] = 0; w2[20 * oc.BW:21 * oc.BW] = 0
        add("clear.%d" % j, base().clear(two), w2)
        add("set.%d" % j, base().clear(two).set(two), w)
        add("keep.%d" % j, base().keep(ids[ids >> 16 != 5].astype(np.uint32)), np.where(np.arange(oc.NW) // oc.BW == 5, 0, w).astype(np.uint32))
        # set_range / clear_range / keep_range: this OP a vector of GAP blocks
        lo, hi = 16 * oc.B + 1000, 18 * oc.B + 2000
        rb = np.zeros(oc.NBITS, bool); rb[lo:hi + 1] = True
        kb = np.zeros(oc.NBITS, bool); kb[1:29 * oc.B + 8] = True
        add("set_range.%d" % j, base().set_range(lo, hi), oc.words_of(bits | rb))
        add("clear_range.%d" % j, base().clear_range(lo, hi), oc.words_of(bits & ~rb))
        add("keep_range.%d" % j, base().keep_range(1, 29 * oc.B + 7), oc.words_of(bits & kb))
        # pairwise results under opt_compress
        b = bm.bit_import_u32(c, wb, True)
        add("bit_or.%d" % j, bm.bvector.bit_or(imp, b, bm.opt_compress), w | wb)
        r_and = add("bit_and.%d" % j, bm.bvector.bit_and(imp, b, bm.opt_compress), w & wb)
        add("bit_xor.%d" % j, bm.bvector.bit_xor(imp, b, bm.opt_compress), w ^ wb)
        r_sub = add("bit_sub.%d" % j, bm.bvector.bit_sub(imp, b, bm.opt_compress), w & ~wb)
        # aggregator results with the optimisation on; result vectors of a results pipeline
        agg.set_optimization(True)
        c_or = add("combine_or.%d" % j, agg.combine_or([imp, b, r_sub]), w | wb)
        agg.set_optimization(False)
        add("combine_and_sub.%d" % j, agg.combine_and_sub([c_or, imp], [b])[0], w & ~wb)
        pipe = bm.aggregator.pipeline(c, bm.agg_run_options(True, True))
        for x, y in ((imp, b), (c_or, b)):
            ag = pipe.add()
            ag.add(x, 0); ag.add(y, 1)
        pipe.complete()
        agg.combine_and_sub(pipe)
        for g, r in enumerate(pipe.get_bv_res_vector()):
            assert r is not None
            add("pipeline result.%d.%d" % (g, j), r, w & ~wb)
        # rank compression with optimize
        rc = bm.rank_compressor(c)
        small = bm.bvector.from_ranges(c, np.array([[3, 40], [50, 50], [60, 300]], np.uint64), 512)
        add("rank_compressor decompress.%d" % j, rc.decompress(imp, small, optimize=True))
        add("rank_compressor compress.%d" % j, rc.compress(imp, r_and, optimize=True))
        # scanner results: the rows whose value is 5 are the pattern's rows (planes 0 and 2)
        sc = bm.slice_scanner(c, [imp, None, imp], size=oc.NBITS)
        add("scanner find_gt.%d" % j, sc.find_gt(3), w)
        add("scanner find_eq.%d" % j, sc.find_eq(5)[0], w)
    # GAP x GAP results that stay GAP blocks as they are: all ones as ONE run, and 1,276 runs (pair_cases: gh | gh2)
    K = pc._classes()

    def col16(b):
        w = np.zeros(oc.NW, np.uint32); w[16 * oc.BW:17 * oc.BW] = oc.words_of(b)
        return bm.bit_import_u32(c, w, True)

    def head16(v):
        kinds, offs, _, g = v.block_table()
        assert kinds[16] == bm.GAP
        return int(g[int(offs[16])]) >> 3, int(g[int(offs[16])]) & 1
    for opt in (bm.opt_none, bm.opt_compress):
        v = add("bit_or one run.%d" % opt, bm.bvector.bit_or(col16(K["g2_0"]), col16(K["g2_1"]), opt))
        assert head16(v) == (1, 1)
        v = add("bit_or 1276 runs.%d" % opt, bm.bvector.bit_or(col16(K["gh"]), col16(K["gh2"]), opt))
        assert head16(v)[0] == oc.MAX_GAP_LEN + 1
    return out


def test_every_gap_writer_is_a_row_operand(port):
    """O6: a list of 64+ vectors out of the products of every writer of a GAP slab, through the row kernel (both depths), the
    column-tile kernel, a prepared OR collection under both builders and a prepared AND collection (combine_and_sub over the
    same list).  Expected: the OR / AND of the operands' own to_words() -- another reader of the same slabs -- and the port's
    result over the downloaded block tables"""
    for build in (0, 1):
        c = bm.context(0)
        agg = bm.aggregator(c)
        try:
            prod = _producers(c, port)
            with_bits = sorted({n.rsplit(".", 1)[0] for n, v in prod if v.info()["counts"][bm.BIT]})
            gap_only = [(n, v) for n, v in prod if not v.info()["counts"][bm.BIT]]
            print("O6 producers, GAP-only:", sorted({n.rsplit(".", 1)[0] for n, v in gap_only}), "with bit-blocks:", with_bits)
            assert set(with_bits) <= set(BIT_BY_DESIGN), with_bits
            assert all(any(k == bm.GAP for k in kinds_of(v)) for n, v in gap_only ), "a GAP block from every producer"
            gv = [v for n, v in gap_only]
            assert len(gv) >= oc.N_ROWS
            words = [v.to_words(oc.NW) for v in gv]
            u, inter = np.bitwise_or.reduce(words, axis=0), None
            pv = [port.from_table(v.info()["nbits"], *v.block_table()) for v in gv]
            for key, x in TABLES: c.set_tuning(key, x)
            seen = {}
            for opt in (False, True):
                agg.set_optimization(opt)
                e = port.agg_or(pv, opt)
                assert (e.to_words(oc.NW) == u).all()
                for path, knobs, first in PATHS[:3]:
                    for key, x in knobs: c.set_tuning(key, x)
                    preconditions(c, gv, path)
                    same(agg.combine_or(gv), u, popcount(u), port_kinds(e), ("O6", build, path, opt))
            # prepared collections: gap_pack at its default, the OR role under this builder, then the AND role
            restore(c)
            for key, x in (("direct_cols", 0), ("pipe_split", 0), ("coll_build", build)): c.set_tuning(key, x)
            c.collection_prepare(gv, bm.ROLE_OR)
            assert c.pack_stats()["collections"] == 1
            for opt in (False, True):
                agg.set_optimization(opt)
                e = port.agg_or(pv, opt)
                same(agg.combine_or(gv), u, popcount(u), port_kinds(e), ("O6", build, "collection", opt))
                c.set_tuning("coll_members", 1)
                h = gv[1::2] + gv[:3]
                eh = port.agg_or(pv[1::2] + pv[:3], opt)
                uh = np.bitwise_or.reduce(words[1::2] + words[:3], axis=0)
                same(agg.combine_or(h), uh, popcount(uh), port_kinds(eh), ("O6", build, "members", opt))
                c.set_tuning("coll_members", -1)
            agg.set_optimization(False)
            full = [(v, p, w) for v, p, w in zip(gv, pv, words) if v.info()["nblocks"] == oc.NBLOCKS]
            c.collection_prepare([v for v, p, w in full], bm.ROLE_AND)
            assert c.pack_stats()["collections"] == 2
            inter = np.bitwise_and.reduce([w for v, p, w in full], axis=0)
            e = port.agg_and_sub([p for v, p, w in full], [])
            assert (e.to_words(oc.NW) == inter).all()
            t, any_ = agg.combine_and_sub([v for v, p, w in full], [])
            same(t, inter, popcount(inter), port_kinds(e), ("O6", build, "and collection"))
            c.set_tuning("coll_members", 1)
            half = [x for x in full[::2]]
            want = np.bitwise_and.reduce([w for v, p, w in half], axis=0) & ~u
            e = port.agg_and_sub([p for v, p, w in half], pv)
            t, any_ = agg.combine_and_sub([v for v, p, w in half], gv)
            same(t, want, popcount(want), port_kinds(e), ("O6", build, "and members, sub collection"))
            assert c.pack_stats()["collections"] == 2
            del t, prod, gap_only, gv, full, half
        finally:
            restore(c)
            del agg
            c.close()
