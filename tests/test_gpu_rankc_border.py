"""GPU: bm::rank_compressor on the device (k_rankc_* of bmx_kernels15.h) on the constructed cases of
tests/golden/rankc_border_cases.py: every border of extract and deposit that tests/test_rankc_border_host.py proves a case meets.
Vectors are built by upload (from_block_table), so the storage kind of every index and source block is the case's.  Per case:
both directions, rankc_path 0, 1 and -1, optimize 0 and 1, with and without the rs index, as one batch (with an absent plane and the
index's own handle among the sources) and singly: size(), count(), to_indices() and the block table byte for byte against the closed
form; tables equal across paths, index forms and batch / single; the round trips; one case through slice_scanner.decompress."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import bitmagic_amd as bm  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import rankc_border_cases as rb  # noqa: E402
from import_cases import canonical, record  # noqa: E402

CASES = rb.cases()
U = np.uint64
_DEV, _PLAN = {}, {}


def _upload(ctx, v):
    dv = bm.bvector.from_block_table(ctx, v.nbits, *v.table())
    assert (dv.block_table()[0] == v.block_kinds()).all() and dv.size() == v.nbits          # stored as the case says
    return dv


def _dev(ctx, name):
    """-> index, its rs index, [(source name, vector)]: uploaded once per session"""
    if name not in _DEV:
        c = CASES[name]
        idx = _upload(ctx, c.idx)
        rs = idx.build_rs_index()
        assert rs.count() == c.idx.count == idx.count()
        _DEV[name] = (idx, rs, [(s, _upload(ctx, v)) for s, v in c.srcs])
    return _DEV[name]


def _table(v):
    return (v.size(),) + tuple(v.block_table())


def _same(a, b):
    return a[0] == b[0] and all(x.dtype == y.dtype and x.shape == y.shape and (x == y).all() for x, y in zip(a[1:], b[1:]))


def _explain(c, direction, sname, got_ids):
    """the case, the first block whose positions differ, and what plan() says the kernel decides there"""
    exp = rb.expected(c, sname, direction)["pos"]
    diff = np.setxor1d(np.asarray(got_ids, U), exp)
    if c.name not in _PLAN: _PLAN[c.name] = rb.plan(c)
    if not diff.size:
        return "%s source %s %s: positions equal, the table differs" % (c.name, sname, direction)
    p = int(diff[0]); blk = p >> 16
    # the (index block, 256-word row) pairs whose bits differ: a rank maps back through the index
    kb = U(c.idx.prefix * rb.B)
    ip = diff if direction == "decompress" else np.concatenate([diff[diff < kb], c.idx.ones[(diff[(diff >= kb) & (diff < U(c.idx.count))] - kb).astype(np.int64)]])
    rows = np.unique(ip >> U(13))
    rows = ["%d.%d" % (int(r) >> 3, int(r) & 7) for r in rows[:24]] + (["..."] if rows.size > 24 else [])
    fields = _PLAN[c.name]["deposit" if direction == "decompress" else "extract"][sname].get(blk)
    return "%s source %s %s: %d positions differ, the first %d (%s) in %s block %d; index block.row of the differing bits: %s; plan: %r; claims: %r" % (
        c.name, sname, direction, diff.size, p, "missing" if p in set(exp[exp >> U(16) == U(blk)].tolist()) else "extra",
        "index" if direction == "decompress" else "target", blk, " ".join(rows), fields, c.claims)


def _check_against_closed_form(c, direction, sname, optimize, v, ctxt):
    e = rb.expected(c, sname, direction)
    rec = e["opt1" if optimize else "opt0"]
    ids = v.to_indices()
    why = lambda: (_explain(c, direction, sname, ids), ctxt)                                   # noqa: E731
    assert v.size() == e["nbits_out"], why()
    assert v.count() == e["count"] and ids.size == e["count"] and (ids == e["pos"]).all(), why()
    kinds, offs, bits, gaps = v.block_table()
    assert record(kinds, offs, bits, gaps) == rec, why()
    # the device writes the canonical layout itself: GAP blocks from 16-byte boundaries, 0xFFFF padding; level bits masked
    k, o, b, g = canonical(kinds, offs, bits, gaps)
    assert (o == offs).all(), why()
    gm = gaps.copy()
    for nb in np.nonzero(kinds == bm.GAP)[0]:
        gm[offs[nb]] &= 0xFFF9
    assert (gm == g).all(), why()
    assert v.info()["counts"] == rec["counts"], why()


@pytest.mark.parametrize("name", sorted(CASES))
def test_constructed_case(ctx, name):
    c = CASES[name]
    idx, rs, srcs = _dev(ctx, name)
    rc = bm.rank_compressor(ctx)
    batch = [v for _, v in srcs]
    batch.insert(1, None)                                                                      # an absent plane
    batch.append(idx)                                                                          # the index's own handle: a copy
    at = {s: i + (i >= 1) for i, (s, _) in enumerate(srcs)}
    own = _table(idx)
    first = {}
    try:
        for path in (0, 1, -1):
            ctx.set_tuning("rankc_path", path)
            for optimize in (False, True):
                for use_rs in (None, rs):
                    ctxt = {"rankc_path": path, "optimize": optimize, "rs": use_rs is not None}
                    outs = {"compress": rc.compress_many(idx, batch, use_rs, optimize),
                            "decompress": rc.decompress_many(idx, batch, use_rs, optimize)}
                    for d, o in outs.items():
                        assert len(o) == len(batch) and o[1] is None, (name, d, ctxt)
                        assert _same(_table(o[-1]), own), (name, d, ctxt)
                        for sname, sv in srcs:
                            key = (d, sname, optimize)
                            got = o[at[sname]]
                            if key not in first:
                                _check_against_closed_form(c, d, sname, optimize, got, ctxt)
                                first[key] = _table(got)
                            elif not _same(_table(got), first[key]):                           # across paths and index forms
                                raise AssertionError(("batch", _explain(c, d, sname, got.to_indices()), ctxt))
                            one = rc.compress_by_source(idx, use_rs, sv, optimize) if d == "compress" else rc.decompress(idx, sv, use_rs, optimize)
                            if not _same(_table(one), first[key]):
                                raise AssertionError(("single", _explain(c, d, sname, one.to_indices()), ctxt))
                    del outs
    finally:
        ctx.set_tuning("rankc_path", -1)
    assert len(first) == 4 * len(srcs)


@pytest.mark.parametrize("name", sorted(CASES))
def test_round_trips(ctx, name):
    """decompress(compress(s)) == s & idx and compress(decompress(t)) == t below count(idx), under both paths"""
    c = CASES[name]
    idx, rs, srcs = _dev(ctx, name)
    rc = bm.rank_compressor(ctx)
    cnt = c.idx.count
    try:
        for path in (0, 1):
            ctx.set_tuning("rankc_path", path)
            for sname, sv in srcs:
                ones = c.src(sname).ones
                back = rc.decompress(idx, rc.compress(idx, sv, True), rs, True)
                assert back.size() == c.idx.nbits and (back.to_indices() == rb.and_positions(c.idx, ones)).all(), (name, sname, path)
                again = rc.compress_by_source(idx, rs, rc.decompress(idx, sv, None, True), True)
                below = ones[ones < U(cnt)]
                assert again.size() == cnt and again.count() == below.size and (again.to_indices() == below).all(), (name, sname, path)
    finally:
        ctx.set_tuning("rankc_path", -1)


def test_scanner_entry(ctx):
    """slice_scanner.decompress is the same deposit: D/kinds, every pair of source kinds under a straddling window"""
    c = CASES["D/kinds"]
    idx, rs, srcs = _dev(ctx, c.name)
    sc = bm.slice_scanner(ctx, [], size=c.idx.nbits, not_null=idx)
    for sname in ("kinds", "ones_on_the_window", "ends_at_sb1"):
        e = rb.expected(c, sname, "decompress")
        for r in (None, rs):
            out = sc.decompress(dict(srcs)[sname], r)
            ids = out.to_indices()
            assert out.size() == e["nbits_out"] and ids.size == e["count"] and (ids == e["pos"]).all(), _explain(c, "decompress", sname, ids)
