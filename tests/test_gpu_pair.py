"""GPU: the pairwise path -- bit_and / or / xor / sub, op2_count, op2_async, count_*, bmx_count_op2_dev, distance_operation -- on the
constructed block-pair cases of tests/golden/pair_cases.py (Grid K: every ordered pair of 18 block classes; Grid L: every border
of a GAP run list; four import flavours; short, long, ragged and partial-block forms; a one-level chain; the result tails).
Every comparison is bit-exact and holds words, kinds and count: against the closed form (words and count from the construction,
kinds from pair_cases.model_kind), against the oracle port, and against the reference's fixture (pair_ref.json) where it holds the
case.  Each operation runs under every kernel the plan can pick for it (k_op2, k_op2_loop, k_op2_stream; k_count_op2, its loop
and stream forms; the distance twins), forced by tuning keys that are restored in a `finally`.  A failure names its cell: grid,
column, classes, flavour.  tests/test_pair_host.py keeps the cases and the model honest on the CPU."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bitmagic_amd as bm
import pair_cases as pc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KNOBS = (("op2_loop", -1), ("op2_nt", 3), ("op2_wgs", 4), ("pair_stream", -1), ("pair_wgs", 1), ("pair_loop", -1), ("pair_nt", 1))
MODES = ("none", "compress")
OPT = (bm.opt_none, bm.opt_compress)
COUNT_FN = (bm.count_and, bm.count_or, bm.count_xor, bm.count_sub)
_DEV, _PORT, _FX = {}, {}, {}
FL_IDS = [pc.flavour_name(fl) for fl in pc.FLAVOURS]


def fixture():
    if not _FX:
        with open(os.path.join(ROOT, "tests", "golden", "pair_ref.json")) as f:
            _FX.update(json.load(f))
    return _FX


def restore(ctx):
    for key, x in KNOBS: ctx.set_tuning(key, x)


def tune(ctx, knobs):
    restore(ctx)
    for key, x in knobs: ctx.set_tuning(key, x)


def port_vec(port, p, side, optimised):
    key = (p.name, side, optimised)
    if key not in _PORT:
        w = p.words(side, optimised)
        _PORT[key] = port.import_words(w, optimised, w.size * 32 - p.cut)
    return _PORT[key]


def dev_vec(ctx, port, p, side, optimised):
    """the port's block table uploaded as it is: the device operand holds exactly the kinds the port holds"""
    key = (p.name, side, optimised)
    if key not in _DEV:
        pv = port_vec(port, p, side, optimised)
        _DEV[key] = bm.bvector.from_block_table(ctx, pv.nbits, *pv.flatten())
    return _DEV[key]


def upload(ctx, pv):
    return bm.bvector.from_block_table(ctx, pv.nbits, *pv.flatten())


def port_kinds(pv, nblocks):
    return np.asarray((pv.flatten()[0].tolist() + [0] * nblocks)[:nblocks], np.int64)


class Case:
    """one pair in one flavour and operand order: the closed form, the device operands, the port's"""

    def __init__(self, ctx, port, p, fl, swap=False, fixture_name=None):
        self.ctx, self.port, self.p, self.fl, self.swap = ctx, port, p, fl, swap
        self.e = pc.Expect(p, fl, swap)
        sides = (1, 0) if swap else (0, 1)
        self.g = [dev_vec(ctx, port, p, s, fl[s]) for s in sides]
        self.pv = [port_vec(port, p, s, fl[s]) for s in sides]
        self.nw = p.nblocks * pc.BW
        self.fx = None if (swap or fixture_name is None) else fixture()["pairs"][fixture_name].get(pc.flavour_name(fl))
        self._want = (None, None)

    def want(self, op, cm):
        """(words, count, kinds, port result) of op under opt mode cm: closed form == port (== fixture), checked here once"""
        if self._want[0] != (op, cm):
            e = self.e
            r, _, cnt = e.result(op)
            r = pc.pad_blocks(r)[:self.nw]
            kinds = e.result_kinds(op, bool(cm))
            pt = self.port.op2(op, self.pv[0], self.pv[1], bool(cm))
            assert pt.count() == cnt and (pt.to_words(self.nw) == r).all(), (e, op, cm, "closed form != port")
            why = pc.first_diff(e, got_kinds=port_kinds(pt, self.p.nblocks), want_kinds=kinds)
            assert why is None, (e, op, cm, "model != port", why)
            if self.fx is not None:
                f = self.fx["%s.%s" % (pc.OP_NAMES[op], MODES[cm])]
                assert (f["count"], f["kinds"]) == (cnt, pc.kinds_str(kinds)) and f["sha"] == pc.sha(r), (e, op, cm, "fixture")
            self._want = ((op, cm), (r, cnt, kinds, pt), {})
        return self._want[1]

    def further(self, op, cm):
        """t ^ (second operand), from the port: (words, kinds)"""
        memo = self._want[2]
        if "x" not in memo:
            u = self.port.op2(pc.XOR, self.want(op, cm)[3], self.pv[1], False)
            memo["x"] = (u.to_words(self.nw), port_kinds(u, self.p.nblocks))
        return memo["x"]

    def check(self, t, op, cm, what, counted=True, handling=True):
        """a device result of op: count() first, then words, kinds; then the result handling (a host block table and back, the
        result as an operand of a count and of one further operation)"""
        e = self.e
        r, cnt, kinds, _ = self.want(op, cm)
        tag = (e, pc.OP_NAMES[op], MODES[cm], what)
        if counted: assert t.count() == cnt, tag + ("count()",)
        i = t.info()
        assert i["nbits"] == max(v.nbits for v in self.pv) and i["nblocks"] == self.p.nblocks, tag
        got = t.to_words(self.nw)
        k, o, bits, gaps = t.block_table()
        why = pc.first_diff(e, got, r, k, kinds)
        assert why is None, tag + (why,)
        assert i["counts"] == np.bincount(kinds, minlength=4).tolist(), tag
        if not handling: return
        back = bm.bvector.from_block_table(self.ctx, i["nbits"], k, o, bits, gaps)
        assert bm.count_xor(t, back) == 0 and bm.count_xor(back, t) == 0 and (back.block_table()[0] == k).all(), tag + ("round trip",)
        assert bm.count_and(t, t) == cnt and bm.count_or(back, t) == cnt, tag + ("as an operand of count_*",)
        xw, xk = self.further(op, cm)
        u = bm.bvector._op2(pc.XOR, t, self.g[1], bm.opt_none)
        why = pc.first_diff(e, u.to_words(self.nw), xw, u.block_table()[0], xk)
        assert why is None, tag + ("result ^ second operand", why)


def both_orders(ctx, port, p, fl, fixture_name=None):
    return [Case(ctx, port, p, fl, False, fixture_name), Case(ctx, port, p, fl, True)]


def flavours_of(name):
    return pc.fixture_pairs()[name][1]


# ---------------------------------------------------------------------------------------------------------------------
# materialised, synchronous
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fl", pc.FLAVOURS, ids=FL_IDS)
def test_short_form(ctx, port, fl):
    """fewer than 2,048 blocks: k_op2, which also folds the count; op2_count with and without a result vector; the partial-block pair"""
    pairs = [(pc.short_pair(), "short")] + ([(pc.cut_pair(), "cut")] if fl in flavours_of("cut") else [])
    try:
        restore(ctx)
        for p, name in pairs:
            for c in both_orders(ctx, port, p, fl, name):
                for op in pc.OPS:
                    for cm in (0, 1):
                        c.check(bm.bvector._op2(op, c.g[0], c.g[1], OPT[cm]), op, cm, "k_op2")
                        t, n = bm.bvector.op2_count(op, c.g[0], c.g[1], OPT[cm], True)
                        assert n == c.want(op, cm)[1], (c.e, op, cm, "op2_count")
                        c.check(t, op, cm, "op2_count", handling=False)
                        assert bm.bvector.op2_count(op, c.g[0], c.g[1], OPT[cm], False) == (None, n), (c.e, op, cm)
    finally:
        restore(ctx)


LOOP_KNOBS = [(("op2_loop", lp), ("op2_nt", nt), ("pair_stream", 0)) for lp in (0, 1, 2, 4, -1) for nt in (0, 3)]


@pytest.mark.parametrize("fl", pc.FLAVOURS, ids=FL_IDS)
def test_long_form_every_loop_shape(ctx, port, fl):
    """2,049 blocks: the persistent kernel at 1, 2, 4 workgroups per CU and its default, the wave-per-column kernel (op2_loop 0), plain
    and non-temporal accesses (pair_stream 0 keeps a pair of raw operands away from the streaming kernel), then the default selection"""
    p = pc.long_pair(pc.FIXTURE_N)
    try:
        for c in both_orders(ctx, port, p, fl, "long%d" % pc.FIXTURE_N):
            for op in pc.OPS:
                for cm in (0, 1):
                    for n, knobs in enumerate(LOOP_KNOBS):
                        tune(ctx, knobs)
                        c.check(bm.bvector._op2(op, c.g[0], c.g[1], OPT[cm]), op, cm, knobs, handling=(n in (0, 3, 9)))
                    restore(ctx)
                    c.check(bm.bvector._op2(op, c.g[0], c.g[1], OPT[cm]), op, cm, "default")
                    t, cnt = bm.bvector.op2_count(op, c.g[0], c.g[1], OPT[cm], True)
                    assert cnt == c.want(op, cm)[1], (c.e, op, cm, "op2_count")
                    c.check(t, op, cm, "op2_count", handling=False)
    finally:
        restore(ctx)


OTHER_LONG = [("long", 2048, 2048)] + [("ragged", a, b) for a, b in pc.RAGGED]


@pytest.mark.parametrize("form,na,nb", OTHER_LONG, ids=["%s%dx%d" % x for x in OTHER_LONG])
def test_long_form_other_lengths(ctx, port, form, na, nb):
    """2,048 blocks (the first length the persistent kernel takes) and the ragged pairs (x op missing), every flavour: the default
    selection, the persistent kernel at one workgroup per CU and the wave-per-column kernel.  (3,073 and 4,097 blocks differ from
    2,049 only in the stretch a wave of the STREAMING kernels owns -- a wave of the persistent kernel strides over the columns
    whatever their number: those lengths run in test_stream_kernel, test_counts and test_distance_operation.)"""
    p = pc.long_pair(na) if form == "long" else pc.ragged_pair(na, nb)
    try:
        for fl in pc.FLAVOURS:
            for c in both_orders(ctx, port, p, fl):
                for op in pc.OPS:
                    for cm in (0, 1):
                        for knobs in ((), (("op2_loop", 1), ("op2_nt", 0), ("pair_stream", 0)), (("op2_loop", 0), ("pair_stream", 0))):
                            tune(ctx, knobs)
                            c.check(bm.bvector._op2(op, c.g[0], c.g[1], OPT[cm]), op, cm, knobs or "default", handling=not knobs)
    finally:
        restore(ctx)


@pytest.mark.parametrize("n", pc.LONG_N)
def test_stream_kernel(ctx, port, n):
    """(raw, raw), equal lengths, opt_none: k_op2_stream.  op2_wgs 1 gives a wave a stretch of 2, 3, 4, 5 columns at the four lengths
    (the two-columns-in-flight loop, its odd and even tails, a short or empty last wave), op2_wgs 4 one or two; plain and
    non-temporal accesses"""
    p = pc.long_pair(n)
    try:
        for c in both_orders(ctx, port, p, (False, False), "long%d" % n if n == pc.FIXTURE_N else None):
            assert all(v.info()["counts"][pc.BIT] == n for v in c.g)
            for op in pc.OPS:
                for wgs in (1, 4):
                    for nt in (0, 3):
                        tune(ctx, (("op2_wgs", wgs), ("op2_nt", nt)))
                        c.check(bm.bvector._op2(op, c.g[0], c.g[1], bm.opt_none), op, 0, ("k_op2_stream", wgs, nt), handling=(wgs == 1))
    finally:
        restore(ctx)


# ---------------------------------------------------------------------------------------------------------------------
# asynchronous
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fl", pc.FLAVOURS, ids=FL_IDS)
def test_async_pairs(ctx, port, fl):
    """op2_async(...).wait() over the short form (with GAP operands: k_op2_loop at any length, laying its GAP results out), the
    partial-block pair, the long form and a ragged pair"""
    pairs = [(pc.short_pair(), "short"), (pc.long_pair(pc.FIXTURE_N), "long%d" % pc.FIXTURE_N), (pc.ragged_pair(*pc.RAGGED[0]), None)]
    if fl in flavours_of("cut"): pairs.append((pc.cut_pair(), "cut"))
    try:
        restore(ctx)
        for p, name in pairs:
            for c in both_orders(ctx, port, p, fl, name):
                for op in pc.OPS:
                    pend = bm.bvector.op2_async(op, c.g[0], c.g[1])
                    c.check(pend.wait(), op, 0, "op2_async")
    finally:
        restore(ctx)


def _chain_port(port):
    """the chain inside the port: name -> vector, for operands and results"""
    p = pc.short_pair()
    a, b = port_vec(port, p, 0, True), port_vec(port, p, 1, True)
    z, o = [port.import_words(w, True, p.nbits) for w in pc.chain_constants()]
    r_or, r_xor = port.op2(pc.OR, a, b, False), port.op2(pc.XOR, a, b, False)
    return p, a, b, z, o, r_or, r_xor


def _check_chain_result(t, first, link, model, p, what):
    f = fixture()["chain"]["%s:%s" % (first, link)]
    lev = model[first, link]
    e = pc.Expect(p, (True, True))
    assert t.count() == f["count"] == int(lev.f[2].sum()), (first, link, what)
    got = t.to_words(p.nblocks * pc.BW)
    k = t.block_table()[0]
    why = pc.first_diff(e, got, lev.w, k, lev.k)
    assert why is None, (first, link, what, why)
    assert pc.sha(got) == f["sha"] and pc.kinds_str(k) == f["kinds"], (first, link, what, "fixture")


@pytest.mark.parametrize("mode", ["sync", "async_reverse_wait", "uploaded_first_level"])
def test_chain(ctx, port, mode):
    """R = A | B, R' = A ^ B, then R & A, R ^ B, R - A, A - R, R | R' and the three copies of R: first-level results hold one-run GAP
    blocks, all-zero bit-blocks, FULL blocks and GAP blocks of 1,276 runs, which no import produces.  sync: every link through
    bmx_op2; async: every link left unresolved until all are enqueued, then waited for in reverse order; uploaded: the port's
    first-level results as host block tables"""
    model, first_model = pc.model_chain()
    p, pa, pb, pz, po, pr_or, pr_xor = _chain_port(port)
    a, b = dev_vec(ctx, port, p, 0, True), dev_vec(ctx, port, p, 1, True)
    z, o = upload(ctx, pz), upload(ctx, po)
    try:
        restore(ctx)
        if mode == "async_reverse_wait":
            r_or, r_xor = bm.bvector.op2_async(pc.OR, a, b), bm.bvector.op2_async(pc.XOR, a, b)
            links = []
            for f in pc.CHAIN_FIRST:
                v = pc.chain_operands(f, a, b, r_or, r_xor, z, o)
                for name, op, x, y in pc.CHAIN_LINKS:
                    links.append((pc.OP_NAMES[f], name, bm.bvector.op2_async(op, v[x], v[y])))
            for f, name, pend in reversed(links):
                _check_chain_result(pend.wait(), f, name, model, p, mode)
            firsts = {"xor": r_xor.wait()}
            firsts["or"] = r_or.wait()
        else:
            if mode == "sync":
                firsts = {"or": bm.bvector._op2(pc.OR, a, b, bm.opt_none), "xor": bm.bvector._op2(pc.XOR, a, b, bm.opt_none)}
            else:
                firsts = {"or": upload(ctx, pr_or), "xor": upload(ctx, pr_xor)}
            for f in pc.CHAIN_FIRST:
                v = pc.chain_operands(f, a, b, firsts["or"], firsts["xor"], z, o)
                for name, op, x, y in pc.CHAIN_LINKS:
                    _check_chain_result(bm.bvector._op2(op, v[x], v[y], bm.opt_none), pc.OP_NAMES[f], name, model, p, mode)
        e = pc.Expect(p, (True, True))
        for f, t in firsts.items():
            lev = first_model[f]
            why = pc.first_diff(e, t.to_words(p.nblocks * pc.BW), lev.w, t.block_table()[0], lev.k)
            assert why is None and t.count() == int(lev.f[2].sum()), (f, mode, why)
    finally:
        restore(ctx)


# ---------------------------------------------------------------------------------------------------------------------
# counts
# ---------------------------------------------------------------------------------------------------------------------
def _count_pairs():
    return [pc.short_pair(), pc.cut_pair()] + [pc.long_pair(n) for n in pc.LONG_N] + [pc.ragged_pair(a, b) for a, b in pc.RAGGED]


COUNT_KNOBS = [(("pair_loop", lp), ("pair_nt", nt), ("pair_stream", 0)) for lp in (0, 2, 3, 4, -1) for nt in (0, 1)]
STREAM_KNOBS = [(("pair_stream", ps), ("pair_wgs", w)) for ps in (0, 2, 4, 8) for w in (1, 4)]


@pytest.mark.parametrize("fl", pc.FLAVOURS, ids=FL_IDS)
def test_counts(ctx, port, fl):
    """count_and / or / xor / sub == the closed form == the port: k_count_op2 (short forms, pair_loop 0), k_count_op2_loop at every
    shape, and for (raw, raw) k_count_op2_stream at 2, 4, 8 waves per workgroup and 1, 4 workgroups per CU; then the default"""
    try:
        for p in _count_pairs():
            if p.cut and fl not in flavours_of("cut"): continue
            for swap in (False, True):
                e = pc.Expect(p, fl, swap)
                sides = (1, 0) if swap else (0, 1)
                ga, gb = [dev_vec(ctx, port, p, s, fl[s]) for s in sides]
                want = [e.count(op) for op in pc.OPS]
                assert want == [port.count_op2(op, *[port_vec(port, p, s, fl[s]) for s in sides]) for op in pc.OPS], e
                for knobs in COUNT_KNOBS + (STREAM_KNOBS if fl == (False, False) else []) + [()]:
                    tune(ctx, knobs)
                    got = [COUNT_FN[op](ga, gb) for op in pc.OPS]
                    assert got == want, (e, knobs or "default", got, want)
    finally:
        restore(ctx)


def test_count_op2_dev_writes_one_slot(ctx, port):
    """bmx_count_op2_dev (the entry bench.py times): the count lands in the slot it was given, in the middle of a pre-filled device
    tensor, and nowhere else; two empty vectors write 0"""
    import torch
    L = bm._ffi.lib()
    FILL = 0x5A5A5A5A5A5A5A5A
    cases = [(pc.short_pair(), (True, True)), (pc.long_pair(2049), (True, False)), (pc.long_pair(2049), (False, False)), (pc.ragged_pair(*pc.RAGGED[1]), (True, True))]
    empty = [bm.bit_import_u32(ctx, np.zeros(0, np.uint32), True) for _ in range(2)]
    assert all(v.info()["nblocks"] == 0 for v in empty)
    try:
        restore(ctx)
        for p, fl in cases:
            e = pc.Expect(p, fl)
            ga, gb = [dev_vec(ctx, port, p, s, fl[s]) for s in (0, 1)]
            buf = torch.full((16,), FILL, dtype=torch.int64, device="cuda")
            torch.cuda.synchronize()
            for op in pc.OPS:
                bm.check(L.bmx_count_op2_dev(ctx._h, op, ga._h, gb._h, C.c_void_p(buf.data_ptr() + 8 * (3 + 2 * op))))
            bm.check(L.bmx_count_op2_dev(ctx._h, pc.XOR, empty[0]._h, empty[1]._h, C.c_void_p(buf.data_ptr() + 8 * 13)))
            ctx.synchronize()
            got = buf.cpu().numpy()
            want = np.full(16, FILL, np.int64)
            for op in pc.OPS: want[3 + 2 * op] = e.count(op)
            want[13] = 0
            assert (got == want).all(), (e, got, want)
    finally:
        restore(ctx)


METRICS = (bm.COUNT_AND, bm.COUNT_XOR, bm.COUNT_OR, bm.COUNT_SUB_AB, bm.COUNT_SUB_BA, bm.COUNT_A, bm.COUNT_B)


@pytest.mark.parametrize("fl", pc.FLAVOURS, ids=FL_IDS)
def test_distance_operation(ctx, port, fl):
    """every metric of bm.distance_operation from one pass (k_distance_pair_loop; (raw, raw) of equal lengths: k_distance_pair_stream
    at 1 and 4 workgroups per CU) == the closed form"""
    try:
        for p in _count_pairs():
            if p.cut and fl not in flavours_of("cut"): continue
            e = pc.Expect(p, fl)
            ga, gb = [dev_vec(ctx, port, p, s, fl[s]) for s in (0, 1)]
            ca, cb = [int(f[2].sum()) for f in e.facts]
            c_and, c_or, c_xor, c_sub = [e.count(op) for op in pc.OPS]
            want = [c_and, c_xor, c_or, c_sub, cb - c_and, ca, cb]
            assert c_or == ca + cb - c_and and c_xor == c_or - c_and and c_sub == ca - c_and
            for wgs in (1, 4):
                tune(ctx, (("pair_wgs", wgs),))
                assert bm.distance_operation(ga, gb, METRICS) == want, (e, wgs)
                assert bm.distance_operation(gb, ga, METRICS[::-1]) == [ca, cb, c_sub, cb - c_and, c_or, c_xor, c_and], (e, wgs, "(B, A)")
                for m, w in zip(METRICS, want):
                    assert bm.distance_operation(ga, gb, [m]) == [w], (e, wgs, m)
    finally:
        restore(ctx)


# ---------------------------------------------------------------------------------------------------------------------
# result tails
# ---------------------------------------------------------------------------------------------------------------------
def _handled(ctx, t, want_dev, kinds, count, tag):
    """content, kinds, count, the block-table round trip and use as an operand of a tail-case result (want_dev: the expected
    vector on the device)"""
    assert t.count() == count, tag
    k, o, bits, gaps = t.block_table()
    assert (k == kinds).all(), tag + (np.flatnonzero(k != kinds)[:8],)
    assert bm.count_xor(t, want_dev) == 0 and bm.count_or(t, want_dev) == count, tag
    back = bm.bvector.from_block_table(ctx, t.info()["nbits"], k, o, bits, gaps)
    assert bm.count_xor(back, want_dev) == 0 and (back.block_table()[0] == k).all(), tag
    assert bm.count_and(t, t) == count and bm.bvector._op2(pc.SUB, t, want_dev, bm.opt_none).count() == 0, tag


@pytest.mark.parametrize("nblocks,ks", pc.SLAB_SPARSE)
def test_slab_sparse_both_sides_of_seven_eighths(ctx, port, nblocks, ks):
    """raw vector AND a mask that is FULL in k columns: k bit-blocks survive in a slab of nblocks slots.  live * 8 < nblocks * 7:
    moved into a right-sized slab (13 of 16, 1,791 of 2,048), else kept (14, 1,792), nothing live: given back (0); the same
    through op2_async, whose wait settles the slab without a layout scan"""
    a, w2 = _sparse_operand(ctx, nblocks)
    try:
        restore(ctx)
        for entry in ("op2", "op2_async"):
            for k in ks:
                mask, cols, m = _sparse_mask(ctx, nblocks, k)
                want = (w2 & m).ravel()
                kinds = np.zeros(nblocks, np.int64)
                kinds[cols] = pc.BIT
                want_dev = bm.bit_import_u32(ctx, want, True)
                t = bm.bvector._op2(pc.AND, a, mask, bm.opt_none) if entry == "op2" else bm.bvector.op2_async(pc.AND, a, mask).wait()
                assert (t.to_words(nblocks * pc.BW) == want).all(), (entry, nblocks, k)
                i = t.info()
                assert i["counts"] == [nblocks - k, 0, k, 0], (entry, nblocks, k)
                assert i["bit_slab_blocks"] == k, (entry, nblocks, k, i)       # (what a download moves: the live blocks, compacted or not)
                _handled(ctx, t, want_dev, kinds, pc.popcount(want), (entry, nblocks, k))
    finally:
        restore(ctx)


def _sparse_operand(ctx, nblocks):
    words = pc.slab_sparse_words(nblocks)
    a = bm.bit_import_u32(ctx, words, False)
    assert a.info()["counts"][pc.BIT] == nblocks
    return a, words.reshape(nblocks, pc.BW)


def _sparse_mask(ctx, nblocks, k):
    cols = pc.slab_sparse_mask(nblocks, k)
    m = np.zeros((nblocks, pc.BW), np.uint32)
    m[cols] = 0xFFFFFFFF
    mask = bm.bit_import_u32(ctx, m.ravel(), True)
    assert mask.info()["counts"][:2] == [nblocks - k, k]
    return mask, cols, m


@pytest.mark.parametrize("entry", ["op2", "op2_async"])
@pytest.mark.parametrize("nblocks", [16, 2048])
def test_slab_compaction_gives_memory_back(ctx, nblocks, entry):
    """ctx.mem_used() after synchronize(); trim() is smaller with the last compacted number of live blocks (13 of 16, 1,791 of
    2,048) than with the first kept one (14, 1,792); no absolute byte numbers.

    What this case found: with the device pool's former granule of 64 KiB (pool_round) a result of 16 blocks added 131,328 bytes
    through op2_async with 13 live blocks and with 14 -- the 13 x 8,192 bytes of the compacted slab occupied the two granules
    of the 16 x 8,192 it was copied out of (bmx_op2: 131,328 against 131,584, the 256 bytes of a kept slab's ordinals).  The
    granule between 64 KiB and 2 MiB is one bit-block now, and the compacted slab is 13 blocks."""
    a, _ = _sparse_operand(ctx, nblocks)
    lo = max(k for k in dict(pc.SLAB_SPARSE)[nblocks] if 0 < k and k * 8 < nblocks * 7)
    used = {}
    try:
        restore(ctx)
        for k in (lo, lo + 1):
            mask = _sparse_mask(ctx, nblocks, k)[0]
            ctx.synchronize(); ctx.trim()
            before = ctx.mem_used()
            t = bm.bvector._op2(pc.AND, a, mask, bm.opt_none) if entry == "op2" else bm.bvector.op2_async(pc.AND, a, mask).wait()
            ctx.synchronize(); ctx.trim()
            used[k] = ctx.mem_used() - before
            assert t.info()["counts"][pc.BIT] == k
            del t
        print("bytes a result of %d / %d live blocks of %d adds (%s):" % (lo, lo + 1, nblocks, entry), used)
        assert used[lo] < used[lo + 1], (entry, nblocks, used)                  # live * 8,192 against nblocks * 8,192
    finally:
        restore(ctx)


@pytest.mark.parametrize("which", pc.TRIM_CASES)
def test_gap_slab_trim(ctx, port, which):
    """the laid-out path (GAP operands, opt_none, 2,048 blocks): no GAP block out -- the GAP slab is given back; 3 out of
    operands that hold 2,048 -- moved into a slab of their size; every block out -- kept; through bmx_op2 and op2_async"""
    p, op = pc.trim_pair(which)
    c = Case(ctx, port, p, (True, True))
    r, cnt, kinds, pt = c.want(op, 0)
    want_dev = upload(ctx, pt)
    try:
        restore(ctx)
        for entry in ("op2", "op2_async"):
            t = bm.bvector._op2(op, c.g[0], c.g[1], bm.opt_none) if entry == "op2" else bm.bvector.op2_async(op, c.g[0], c.g[1]).wait()
            c.check(t, op, 0, (which, entry))
            _handled(ctx, t, want_dev, kinds, cnt, (which, entry))
            gw = t.info()["gap_words"]
            ngap = int((kinds == pc.GAP).sum())
            assert (gw == 0) == (ngap == 0) and gw <= ngap * 712, (which, entry, gw)          # (a block of gA: 702 words, padded to 704)
    finally:
        restore(ctx)


@pytest.mark.parametrize("n_cand", [80, 81])
def test_loop_tail_candidate_list(ctx, n_cand):
    """op2_loop 1: 256 workgroups of 4 waves, workgroup 0 owns columns {0..3} + 1024 k.  Two vectors of 20,481 blocks, NULL but for
    those columns, where A holds gA and B holds dfew: every result there is a GAP candidate, so workgroup 0 parks exactly 80 (its
    list is full) or 81 (the overflow path: it finds them again through st[] / gap_offs[]); through bmx_op2 and op2_async"""
    nbits = pc.TAIL_NBLOCKS * pc.B
    a = bm.bvector.from_ranges(ctx, pc.tail_ranges(n_cand, 0), nbits)
    b = bm.bvector.from_ranges(ctx, pc.tail_ranges(n_cand, 1), nbits)
    cols = np.asarray(pc.tail_columns(n_cand))
    assert a.info()["counts"] == [pc.TAIL_NBLOCKS - n_cand, 0, 0, n_cand] == b.info()["counts"]
    try:
        tune(ctx, (("op2_loop", 1),))
        for op in pc.OPS:
            _, w, cnt = pc.tail_expect(n_cand, op)
            bits = np.unpackbits(w.view(np.uint8), bitorder="little").astype(bool)
            g = pc.gap_words(bits)
            d = np.diff(np.concatenate([[0], bits.astype(np.int8), [0]]))
            lo, hi = np.flatnonzero(d == 1).astype(np.uint64), (np.flatnonzero(d == -1) - 1).astype(np.uint64)
            base = cols.astype(np.uint64) * np.uint64(pc.B)
            want_dev = bm.bvector.from_ranges(ctx, np.stack([(base[:, None] + lo[None, :]).ravel(), (base[:, None] + hi[None, :]).ravel()], axis=1), nbits)
            kinds = np.zeros(pc.TAIL_NBLOCKS, np.int64)
            kinds[cols] = pc.GAP
            for entry in ("op2", "op2_async"):
                t = bm.bvector._op2(op, a, b, bm.opt_none) if entry == "op2" else bm.bvector.op2_async(op, a, b).wait()
                _handled(ctx, t, want_dev, kinds, cnt, (n_cand, pc.OP_NAMES[op], entry))
                k, o, _, gaps = t.block_table()
                for c in cols:                              # every GAP block word for word, wherever the cursor put it
                    assert (gaps[int(o[c]):int(o[c]) + g.size] == g).all(), (n_cand, pc.OP_NAMES[op], entry, "column %d" % c)
    finally:
        restore(ctx)


# ---------------------------------------------------------------------------------------------------------------------
# red zones
# ---------------------------------------------------------------------------------------------------------------------
_REDZONE_SCRIPT = r'''
import json, os, sys
sys.path.insert(0, os.getcwd())
sys.path.insert(0, os.path.join(os.getcwd(), "tests", "golden"))
import numpy as np
import bitmagic_amd as bm
import pair_cases as pc
ctx = bm.context(0)
out = {"enabled": ctx.redzone_check()["enabled"], "ok": True, "bad": []}
def same(t, e, op, what):
    r, _, cnt = e.result(op)
    n = e.pair.nblocks * pc.BW
    if not (t.count() == cnt and (t.to_words(n) == pc.pad_blocks(r)[:n]).all()):
        out["ok"] = False; out["bad"].append(what)
# Grid L (and K): the short form, optimised operands, both entries, both modes
p = pc.short_pair()
e = pc.Expect(p, (True, True))
a, b = [bm.bit_import_u32(ctx, p.words(s, True), True) for s in (0, 1)]
for op in pc.OPS:
    same(bm.bvector._op2(op, a, b, bm.opt_none), e, op, ("short", op, "none"))
    same(bm.bvector._op2(op, a, b, bm.opt_compress), e, op, ("short", op, "compress"))
    same(bm.bvector.op2_async(op, a, b).wait(), e, op, ("short", op, "async"))
    if bm._count_op2(op, a, b) != e.count(op): out["ok"] = False; out["bad"].append(("short", op, "count"))
# the 80 / 81 candidates of one workgroup
ctx.set_tuning("op2_loop", 1)
for n_cand in (80, 81):
    nbits = pc.TAIL_NBLOCKS * pc.B
    a, b = [bm.bvector.from_ranges(ctx, pc.tail_ranges(n_cand, s), nbits) for s in (0, 1)]
    for op in pc.OPS:
        cnt = pc.tail_expect(n_cand, op)[2]
        for t in (bm.bvector._op2(op, a, b, bm.opt_none), bm.bvector.op2_async(op, a, b).wait()):
            if t.count() != cnt or t.info()["counts"][pc.GAP] != n_cand: out["ok"] = False; out["bad"].append(("tail", n_cand, op))
ctx.set_tuning("op2_loop", -1)
# the stream at 4,097 blocks, a stretch of 5 columns per wave
p = pc.long_pair(4097)
e = pc.Expect(p, (False, False))
a, b = [bm.bit_import_u32(ctx, p.words(s, False), False) for s in (0, 1)]
for wgs in (1, 4):
    ctx.set_tuning("op2_wgs", wgs); ctx.set_tuning("pair_wgs", wgs)
    for op in pc.OPS:
        same(bm.bvector._op2(op, a, b, bm.opt_none), e, op, ("stream", wgs, op))
        if bm._count_op2(op, a, b) != e.count(op): out["ok"] = False; out["bad"].append(("stream count", wgs, op))
ctx.synchronize()
out["hits"] = ctx.redzone_check()["hits"]
print("REDZONE " + json.dumps(out))
'''


def test_red_zones_clean():
    """a fresh process under BMX_DEBUG_REDZONE=1: Grid L through every entry, the 80 / 81 parked candidates and the stream at 4,097
    blocks write nothing outside their allocations"""
    env = dict(os.environ, BMX_DEBUG_REDZONE="1")
    r = subprocess.run([sys.executable, "-c", _REDZONE_SCRIPT], capture_output=True, text=True, timeout=600, cwd=ROOT, env=env)
    line = [l for l in r.stdout.splitlines() if l.startswith("REDZONE ")]
    assert r.returncode == 0 and line, (r.stdout + r.stderr)[-3000:]
    out = json.loads(line[0][8:])
    assert out["enabled"] and out["hits"] == 0, out
    assert out["ok"], out
