"""GPU: the AND / AND-SUB fold at every threshold of its kernels, on constructed cases (tests/golden/and_fold_cases.py: grids G1 ..
G5, each case one decision point of ar_union_list, gap_apply_list, gap_apply_sparse, sparse_test or pipe_chain, with its
answer in closed form; tests/test_and_fold_host.py keeps the generator honest on the CPU).  Every comparison is bit-exact,
against the closed form and against the oracle port:
  combine_and_sub + find_first_and_sub   words of all three blocks, block kinds, any; found and position; both list paths
  counts pipelines                       the case's group, the AND list reversed, the SUB list dropped -- under every kernel the
                                         plan can pick for the operand kinds, each forced and named by pipe.describe()
  combine_and_sub_indices                the hits of the same pipelines, at width 4 and 8 (k_pipe_hit_counts, bmx_kernels16.h)
A failure names its case: n_and, n_sub, d (killer index), P (shared bits), e (operands carrying the layer L), len, start bit."""
import numpy as np
import pytest

import and_fold_cases as fc
import bitmagic_amd as bm

pytestmark = pytest.mark.gpu

_PV, _GV = {}, {}
NW3 = fc.NBLOCKS * fc.BW
KNOBS = (("and_rows", -1), ("and_rows_wg", 256), ("and_rows_ipw", 0), ("gap_count", -1), ("pipe_split", -1), ("pipe_staged", -1),
         ("pipe_unroll", 0), ("pipe_rows", 0), ("direct_cols", 384))


def _vecs(ctx, port, ops):
    return [fc.device_vec(bm, ctx, port, o, _GV, _PV) for o in ops], [fc.port_vec(port, o, _PV) for o in ops]


@pytest.mark.parametrize("grid,k", fc.chunks())
def test_list_calls(ctx, port, grid, k, agg_path):
    """aggregator.combine_and_sub(and list, sub list) and find_first_and_sub over every case of the chunk"""
    agg = bm.aggregator(ctx)
    for c in fc.chunk(grid, k):
        (ga, pa), (gs, ps) = _vecs(ctx, port, c.ands), _vecs(ctx, port, c.subs)
        e = port.agg_and_sub(pa, ps)
        t, any_ = agg.combine_and_sub(ga, gs)
        got = t.to_words(NW3)
        assert (got == c.expect_words).all(), (agg_path, c, "blocks that differ from the closed form", np.unique(np.flatnonzero(got != c.expect_words) // fc.BW))
        assert (got == e.to_words(NW3)).all(), (agg_path, c)
        assert t.block_table()[0].tolist() == (e.flatten()[0].tolist() + [0] * fc.NBLOCKS)[:t.info()["nblocks"]], (agg_path, c)
        assert any_ == (c.expect_count != 0), (agg_path, c)
        found, pos = agg.find_first_and_sub(ga, gs)
        (ef, epos), (pf, ppos) = c.first(), port.find_first_and_sub(pa, ps)
        assert found == ef == pf and (not found or pos == epos == ppos), (agg_path, c, found, pos, epos)


def _pipeline(ctx, port, cases):
    """one counts pipeline for the cases: per case its group, the group with the AND list reversed, the group without its SUB list"""
    pipe = bm.aggregator.pipeline(ctx)
    groups = []
    for c in cases:
        (ga, pa), (gs, ps) = _vecs(ctx, port, c.ands), _vecs(ctx, port, c.subs)
        for a, s, p in ((ga, gs, (pa, ps)), (ga[::-1], gs, (pa[::-1], ps)), (ga, [], (pa, []))):
            ag = pipe.add()
            for x in a: ag.add(x, 0)
            for x in s: ag.add(x, 1)
            groups.append(p)
    pipe.complete()
    exp = port.pipeline_counts(groups)
    for i, c in enumerate(cases):                           # the closed form, for the two groups it covers
        assert int(exp[3 * i]) == int(exp[3 * i + 1]) == c.expect_count, c
    return pipe, groups, exp


def _forced(ctx, kind, grid):
    """(tuning keys, text pipe.describe() must hold or None) of every counts kernel the plan can pick for the operand kinds"""
    if kind == "gap":
        out = []
        if grid == "G1":                                    # the row kernel's workgroup sizes (2, 4, 8 waves deal the operands) and items per workgroup
            for wg in (128, 256, 512):
                for ipw in (1, 3):
                    out.append(((("and_rows", 1), ("pipe_split", 0), ("and_rows_wg", wg), ("and_rows_ipw", ipw)), "k_agg_and_rows<COUNT,%d," % wg))
        else:
            out.append(((("and_rows", 1), ("pipe_split", 0)), "k_agg_and_rows<COUNT,"))
        # (pipe_split 0: few items with long lists would take the workgroup-split kernel before either of these)
        out.append(((("and_rows", 0), ("gap_count", 1), ("pipe_split", 0)), "k_pipe_counts_gapcount"))
        out.append(((("and_rows", 0), ("gap_count", 0), ("pipe_split", 1)), "k_pipe_split"))
        out.append(((("and_rows", 0), ("gap_count", 0), ("pipe_split", 0)), "k_pipe_counts<"))
        return out
    if kind == "bit":
        # (slices in flight x slice size: the shapes of test_launch_shape_knobs_do_not_change_results; 8 in flight exists for slices of <= 4 KiB)
        return [((("pipe_unroll", u), ("pipe_rows", rows), ("pipe_split", 0)), "k_pipe_counts_bits2<%d," % u) for rows, u in ((8, 4), (4, 8), (1, 8), (1, 4))] + \
               [((("pipe_split", 0),), "k_pipe_counts_bits2<")]
    return [((("direct_cols", 0),), None)]


@pytest.mark.parametrize("grid,k", fc.chunks())
def test_pipelines(ctx, port, grid, k):
    """counts and index lists of the chunk's cases, one pipeline per operand kind, under every kernel of that kind"""
    agg = bm.aggregator(ctx)
    cases = fc.chunk(grid, k)
    for kind in ("gap", "bit", "mixed"):
        some = [c for c in cases if c.kind == kind]
        if not some: continue
        pipe, groups, exp = _pipeline(ctx, port, some)

        def check(got, what):
            bad = np.flatnonzero(np.asarray(got) != exp)
            assert not bad.size, (what, some[bad[0] // 3], "group %d of the case (0: as is, 1: AND list reversed, 2: no SUB list)" % (bad[0] % 3),
                                  int(got[bad[0]]), int(exp[bad[0]]))
        try:
            for knobs, text in _forced(ctx, kind, grid):
                for key, x in KNOBS: ctx.set_tuning(key, x)
                ctx.set_tuning("pipe_staged", 0)            # (many groups over few vectors would take the LDS-staged kernel)
                for key, x in knobs: ctx.set_tuning(key, x)
                d = pipe.describe()
                if text is not None: assert text in d, (knobs, d)
                check(agg.combine_and_sub(pipe), (knobs, d))
            for key, x in KNOBS: ctx.set_tuning(key, x)     # the default selection
            check(agg.combine_and_sub(pipe), ("default", pipe.describe()))
            # index lists of block column 1, the one that carries the cases (block 0 alone would be 49,001 hits per group)
            want3 = []
            for pa, ps in groups[2::3]:
                w = port.agg_and_sub(pa, ps).to_words(NW3)[fc.BW:2 * fc.BW]
                want3.append(np.flatnonzero(np.unpackbits(w.view(np.uint8), bitorder="little")) + fc.B)
            for width in (4, 8):
                off, ids = agg.combine_and_sub_indices(pipe, 1, 2, width=width)
                assert off.size == 3 * len(some) + 1 and int(off[-1]) == ids.size, (width, some[0])
                for i, c in enumerate(some):
                    want = np.flatnonzero(c.expect1) + fc.B
                    for g, w in ((3 * i, want), (3 * i + 1, want), (3 * i + 2, want3[i])):
                        got = ids[int(off[g]):int(off[g + 1])]
                        assert got.size == w.size and (got == w).all(), (width, c, "group %d of the case" % (g % 3), got[:8], w[:8])
        finally:
            for key, x in KNOBS: ctx.set_tuning(key, x)
