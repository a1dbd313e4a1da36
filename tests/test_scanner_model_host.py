"""CPU: the integer model of the comparison search (tests/golden/scanner_cmp_cases.py) against the reference's results, and the
columns it generates against what they claim to hold.

1. The model -- row i matches iff it is not NULL, i < size and the predicate holds in plain integer arithmetic -- reproduces
   the count and the content hash of every cmp / range / zero / nonzero entry of golden_ref.json["scanner"], which
   bm::sparse_vector_scanner<> wrote for an unsigned and an int container, with and without NULL rows.
2. s2u / u2s are inverse to each other on the whole 64-bit range.
3. Each generated column holds the block kinds its test needs, read from the oracle port's block table."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import scanner_cmp_cases as sc  # noqa: E402
from cases import scanner_values, scanner_values_signed, sha  # noqa: E402

PREDS = {"gt": sc.GT, "ge": sc.GE, "lt": sc.LT, "le": sc.LE, "eq": sc.EQ}
ALL_KINDS = {sc.NULL, sc.FULL, sc.GAP, sc.BIT}


@pytest.mark.parametrize("section", ["no_null", "with_null", "signed_no_null", "signed_with_null"])
def test_model_reproduces_the_reference_fixture(golden, section):
    g = golden["scanner"][section]
    signed, with_null = section.startswith("signed"), section.endswith("with_null")
    vals, isn = (scanner_values_signed if signed else scanner_values)(with_null)
    assert sha(vals) == g["values_sha"]
    values = vals.astype(np.int64 if signed else np.uint64)
    valid = None if isn is None else isn == 0
    n = g["rows"]
    nw = (n + 31) // 32

    def chk(bits, e):
        assert int(bits.sum()) == e["count"] and sha(sc.pack(bits, nw)) == e["sha"], e

    seen = 0
    for name, pred in PREDS.items():
        for e in g["cmp"][name]:
            chk(sc.expect(pred, e["v"], 0, values, valid, n), e)
            seen += 1
    for e in g["range"]:
        chk(sc.expect(sc.RANGE, e["from"], e["to"], values, valid, n), e)
    chk(sc.expect(sc.ZERO, 0, 0, values, valid, n), g["zero"])
    chk(sc.expect(sc.NONZERO, 0, 0, values, valid, n), g["nonzero"])
    assert seen == 5 * len(g["cmp"]["gt"]) and seen >= 80 and len(g["range"]) >= 8
    # the planes the model builds are the planes the reference held
    pl = sc.planes(values, signed, g["effective_slices"])
    for p, c in zip(pl, g["plane_counts"]):
        assert (0 if p is None else int(p.sum())) == (c or 0)


def test_sign_encoding_round_trips():
    rng = np.random.default_rng(7)
    fixed = [0, 1, -1, 2, -2, sc.I64_MAX, sc.I64_MIN, sc.I64_MAX - 1, sc.I64_MIN + 1, 1 << 40, -(1 << 40)]
    rand = rng.integers(sc.I64_MIN, sc.I64_MAX, 4000, dtype=np.int64, endpoint=True)
    for v in fixed + [int(x) for x in rand]:
        u = sc.s2u(v)
        assert 0 <= u <= sc.U64_MAX and sc.u2s(u) == v
    assert [sc.s2u(v) for v in (0, -1, 1, -2, 5, -3, sc.I64_MAX, sc.I64_MIN)] == [0, 1, 2, 3, 10, 5, sc.U64_MAX - 1, sc.U64_MAX]
    arr = np.concatenate([np.array(fixed, np.int64), rand])
    u = sc.s2u_array(arr)
    assert [int(x) for x in u[:64]] == [sc.s2u(int(v)) for v in arr[:64]]
    assert (sc.u2s_array(u) == arr).all()
    ur = rng.integers(0, sc.U64_MAX, 4000, dtype=np.uint64, endpoint=True)
    assert (sc.s2u_array(sc.u2s_array(ur)) == ur).all() and sc.s2u(sc.u2s(sc.U64_MAX)) == sc.U64_MAX


def test_model_edges():
    """bounds outside the array's type, a reversed range, rows past the values, rows past size"""
    v = np.array([sc.I64_MIN, -1, 0, 1, sc.I64_MAX], np.int64)
    assert sc.expect(sc.GT, sc.I64_MIN, 0, v, None, 5).tolist() == [False, True, True, True, True]
    assert sc.expect(sc.LE, sc.I64_MIN, 0, v, None, 5).tolist() == [True, False, False, False, False]
    assert sc.expect(sc.GT, sc.I64_MAX + 1, 0, v, None, 5).sum() == 0 and sc.expect(sc.LT, sc.I64_MAX + 1, 0, v, None, 5).all()
    assert sc.expect(sc.GE, sc.I64_MIN - 1, 0, v, None, 5).all()
    assert sc.expect(sc.RANGE, 1, -1, v, None, 5).tolist() == [False, True, True, True, False]
    assert sc.expect(sc.ZERO, 0, 0, v, None, 7).tolist() == [False, False, True, False, False, True, True]      # rows past the values hold 0
    valid = np.array([True, True, False, True, True])
    assert sc.expect(sc.ZERO, 0, 0, v * valid, valid, 7).sum() == 0                                             # ... and are NULL
    assert sc.expect(sc.NONZERO, 0, 0, v, None, 2).tolist() == [True, True]
    u = np.array([0, 1, 1 << 63, sc.U64_MAX], np.uint64)
    assert sc.expect(sc.GE, 1 << 63, 0, u, None, 4).tolist() == [False, False, True, True]
    assert sc.expect(sc.LT, -1, 0, u, None, 4).sum() == 0


def _kinds(port, bits):
    """the block kinds the oracle stores an operand with (what the GPU test uploads)"""
    nbits = bits.size
    nblk = (nbits + sc.B - 1) // sc.B
    return [int(k) for k in port.import_words(sc.pack(bits, nblk * 2048), True, nbits).flatten()[0]]


def _column_kinds(port, col):
    pl, nn = col.operands()
    return [None if p is None else _kinds(port, p) for p in pl], (None if nn is None else _kinds(port, nn))


def test_kind_grids_hold_every_block_kind(port):
    for gen, signed in ((sc.kinds_signed64, True), (sc.kinds_unsigned64, False)):
        col = gen(True)
        pk, nk = _column_kinds(port, col)
        lead = pk[0] if signed else pk[63]                     # the plane that follows the kind plan: the sign / the top plane
        rest = [k for i, k in enumerate(pk) if k is not None and k is not lead]
        assert len(pk) == 64 and all(k is not None for k in pk), col.name
        assert set(lead) == ALL_KINDS and set(nk) == ALL_KINDS, (col.name, lead, nk)
        assert {k for p in rest for k in p} == ALL_KINDS, col.name
        # the LDS reuse case of the half-block kernel: a GAP lead block, a GAP not-NULL block and a GAP magnitude block in one column
        shared = [b for b in range(sc.GRID_BLOCKS) if lead[b] == sc.GAP and nk[b] == sc.GAP and any(p[b] == sc.GAP for p in rest)]
        assert shared, col.name
        # NULL rows hold +0: the sign is a subset of the not-NULL vector
        assert not col.values[~col.valid].any()
        # without a not-NULL vector the plan's kinds are free: a FULL lead block over bit, GAP, FULL and NULL magnitude blocks
        free = gen(False)
        fk, none = _column_kinds(port, free)
        assert none is None and len(fk) == (65 if signed else 64) and (not signed or fk[64] is None)
        flead = fk[0] if signed else fk[63]
        assert flead == [sc.KIND_OF_CODE[b & 3] for b in range(sc.GRID_BLOCKS)], free.name
        frest = [k for k in fk if k is not None and k is not flead]
        for b in (1, 5, 9, 13):
            assert flead[b] == sc.FULL and {p[b] for p in frest} >= {sc.BIT, sc.GAP, sc.FULL}, (free.name, b)
        assert {k for p in frest for k in p} == ALL_KINDS
    s = sc.kinds_signed64(True)
    for x in (sc.I64_MIN, sc.I64_MAX, -1, 0, 1):
        assert ((s.values == x) & s.valid).any(), x
    u = sc.kinds_unsigned64(True)
    for x in (sc.U64_MAX, 1 << 63, (1 << 63) - 1):
        assert ((u.values == np.uint64(x)) & u.valid).any(), x
    assert s.size == u.size == 16 * sc.B - 77


def test_narrow_and_short_columns_are_what_they_claim(port):
    for wn in (True, False):
        c = sc.narrow_signed("plane4_absent", wn)
        pl, _ = c.operands()
        assert len(pl) == 11 and pl[4] is None and all(p is not None for i, p in enumerate(pl) if i != 4)
        c = sc.narrow_signed("sign_absent", wn)
        pl, _ = c.operands()
        assert pl[0] is None and all(p is not None for p in pl[1:]) and (c.values >= 0).all()
        c = sc.narrow_signed("sign_only", wn)
        pl, _ = c.operands()
        assert len(pl) == 1 and pl[0] is not None and set(np.unique(c.values).tolist()) == {0, -1}
        c = sc.narrow_signed("no_planes", wn)
        assert c.operands()[0] == [] and not c.values.any()
        assert c.size == 3 * sc.B + 999
    for signed in (True, False):
        c = sc.short_operands(signed, True)
        pk, nk = _column_kinds(port, c)
        nblk = (c.size + sc.B - 1) // sc.B
        assert nblk == 6 and len(pk[0]) == 2 and len(nk) == 3 and len(pk[5]) == 1
        assert all(len(p) == nblk for i, p in enumerate(pk) if i not in (0, 5))
        # what the cut operands spell is what the model sees: a plane rebuilt at full length has nothing past the cut
        full = sc.planes(c.values, signed, c.nplanes)
        assert not full[0][2 * sc.B:].any() and not full[5][sc.B:].any() and not c.valid[3 * sc.B:].any()
        assert full[0][:2 * sc.B].any() and full[5][:sc.B].any() and not c.values[3 * sc.B:].any()
        free = sc.short_operands(signed, False)
        assert free.valid is None and free.values[3 * sc.B:].any() and "nn" not in free.lengths
        if signed:
            assert (c.values[2 * sc.B:] >= 0).all() and (c.values[:2 * sc.B] < 0).any()


def test_bounds_and_ranges_cover_both_sides_of_zero_and_the_extremes():
    for name, make in sc.all_columns().items():
        col = make()
        lo, hi = col.type_range()
        b, r = sc.bounds(col), sc.ranges(col)
        assert {lo, hi, 0, 1, 2} <= set(b) and all(lo <= x <= hi for x in b), name
        present = sc.present_values(col)
        assert present and all(col.expect(sc.EQ, p).any() for p in present), name
        assert set(present) <= set(b)
        if col.signed:
            assert {-1, -2} <= set(b)
            assert any(x < 0 and y < 0 and x != y for x, y in r) and any(x < 0 < y for x, y in r) and (lo, -1) in r and (-1, 0) in r
            if col.nplanes < 41:
                assert {1 << 40, -(1 << 40)} <= set(b)
            if col.nplanes >= 64:
                assert {sc.I64_MIN, sc.I64_MIN + 1, sc.I64_MAX} <= set(b)
        assert any(x > y for x, y in r) and any(x == y for x, y in r) and (lo, hi) in r and (0, hi) in r, name
