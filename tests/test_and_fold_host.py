"""CPU: the constructed cases of the AND / AND-SUB fold (tests/golden/and_fold_cases.py) are what they claim to be.  Every operand
imports to the block kinds, the run count and the start bit it was built for; the closed form of every case equals the
oracle port's agg_and_sub, pipeline count and find_first_and_sub -- and the reference's on a fixed tenth of the cases, where
the reference is built.  The GPU module (tests/test_gpu_and_fold.py) compares the kernels with the same cases."""
import numpy as np
import pytest

import and_fold_cases as fc
import oracle

_PV = {}


def port_vec(orc, op):
    return fc.port_vec(orc, op, _PV)


def check_operand(port, op):
    kinds, offs, _, gaps = port_vec(port, op).flatten()
    assert tuple(int(k) for k in kinds) == op.kinds, (op.note, kinds, op.kinds)
    for b in range(fc.NBLOCKS):
        if op.kinds[b] == fc.GAP:
            g = op.gaps[b]
            got = gaps[int(offs[b]):int(offs[b]) + g.size]
            assert (got == g).all(), (op.note, b, got[:4], g[:4])       # header (len, level, start bit) and every run end
    g = op.gaps[1]
    if g is not None:
        assert (int(g[0]) >> 3, int(g[0]) & 1) == (op.len1, op.sbit1)
    if op.table:
        # what an import makes of the same bits: the same GAP block, unless it is one run (then NULL / FULL, which is why the
        # operand is uploaded as a table)
        k2, o2, _, g2 = port.import_words(op.words, True, fc.NBITS).flatten()
        if op.len1 == 1:
            assert int(k2[1]) == (fc.FULL if op.sbit1 else fc.NULL)
        else:
            assert int(k2[1]) == fc.GAP and (g2[int(o2[1]):int(o2[1]) + op.gaps[1].size] == op.gaps[1]).all()


def check_case(orc, c, operands_too):
    ops = {o.uid: o for o in c.ands + c.subs}
    if operands_too:
        for o in ops.values():
            check_operand(orc, o)
        k1 = {o.kinds[1] for o in c.ands + c.subs}
        if c.kind == "gap": assert k1 <= {fc.GAP, fc.FULL} and fc.BIT not in {k for o in ops.values() for k in o.kinds}, c
        if c.kind == "bit": assert {k for o in ops.values() for k in o.kinds} == {fc.BIT}, c
        if c.kind == "mixed": assert k1 == {fc.GAP, fc.BIT}, c
        if c.under_test is not None:
            assert (c.under_test.len1, c.under_test.sbit1) == (c.params["len"], c.params["sbit"]), c
    a, s = [port_vec(orc, o) for o in c.ands], [port_vec(orc, o) for o in c.subs]
    r = orc.agg_and_sub(a, s)
    assert (r.to_words(fc.NBLOCKS * fc.BW) == c.expect_words).all(), c
    assert int(orc.pipeline_counts([(a, s)])[0]) == c.expect_count, c
    found, pos = orc.find_first_and_sub(a, s)
    ef, epos = c.first()
    assert found == ef and (not found or pos == epos), (c, found, pos, ef, epos)


def test_largest_gap_block_an_import_keeps(port):
    """G1 reaches up to the longest run list the importer still stores as a GAP block: found by importing, one run more is a bit-block"""
    kinds = {}
    for ln in range(fc.MAX_GAP_LEN - 3, fc.MAX_GAP_LEN + 4):
        for sb in (0, 1):
            b = fc.block_with_len(ln, sb)
            assert fc.len_sbit(b) == (ln, sb)
            k, _, _, g = port.import_words(fc.words_of(b), True, fc.B).flatten()
            kinds[ln, sb] = int(k[0])
            if int(k[0]) == fc.GAP: assert int(g[0]) >> 3 == ln and int(g[0]) & 1 == sb
    largest = max(ln for (ln, sb), k in kinds.items() if k == fc.GAP)
    print("largest len kept as GAP:", largest)
    assert largest == fc.MAX_GAP_LEN and all((k == fc.GAP) == (ln <= largest) for (ln, sb), k in kinds.items())
    assert max(fc.g1_lens()) == largest


def test_grids_cover_what_they_name():
    """the grids hold the values they are laid around (the constants restate bmx_device.h / bmx_kernels9.h)"""
    g1 = fc.grid("G1")
    piece = fc.PIECE_CHUNKS * fc.CHUNK_WORDS
    for lo in (1, 9, piece - 8, 2 * piece - 8, fc.MAX_GAP_LEN - 7):       # every residue mod 8, both start bits, 1 / 2 / 3 pieces
        seen = {(c.params["len"], c.params["sbit"], c.name.endswith("/and")) for c in g1 if c.name.startswith("len")}
        assert all((ln, sb, role) in seen for ln in range(lo, lo + 8) for sb in (0, 1) for role in (True, False)), lo
    assert {c.params["n_and"] for c in fc.grid("G2")} == set(fc.N_AND)
    assert {c.params["n_sub"] for c in fc.grid("G2")} == set(fc.N_SUB)
    g3 = fc.grid("G3")
    for n in fc.N_AND:
        ds = {c.params["d"] for c in g3 if c.params["n_and"] == n and c.kind == "gap" and c.params["d"] is not None}
        assert {0, min(1, n - 1), n - 1} <= ds and all(m in ds for m in range(0, n, 4)), n
    assert {c.params["n_and"] for c in g3 if c.kind == "bit"} >= set(range(1, 2 * 2 * fc.PIPE_U + 2))
    assert {c.params["P"] for c in fc.grid("G4")} == set(fc.P_GRID) and fc.SPARSE_CAP + 1 in fc.P_GRID
    assert all(64 * nj in fc.P_GRID and 64 * nj + 1 in fc.P_GRID for nj in fc.NJ_BUCKETS if nj > 1)
    assert {c.params["e"] for c in fc.grid("G5") if c.params["n_and"] == 12} >= {1, 2, fc.HEAD - 1, fc.HEAD, 10, 11}
    assert {c.params["e"] for c in fc.grid("G5") if c.params["n_and"] == 137} >= {fc.HEAD, fc.HEAD + 1, fc.HEAD + fc.LANE_STEP, fc.HEAD + fc.LANE_STEP + 1, 135}
    print("cases per grid:", {g: len(fc.grid(g)) for g in fc.N_CASES})


@pytest.mark.parametrize("grid,k", fc.chunks())
def test_closed_form_equals_the_oracle(port, grid, k):
    for c in fc.chunk(grid, k):
        check_case(port, c, True)


@pytest.mark.skipif(not oracle.have_reference("avx2"), reason="needs the reference build (oracle/_ref)")
def test_closed_form_equals_the_reference_on_a_tenth():
    ref = oracle.reference("avx2")
    n = 0
    for g in fc.N_CASES:
        for c in fc.grid(g)[3::10]:
            check_case(ref, c, False)
            n += 1
    assert n > 300
