"""GPU: build_rs_index, rank and select on the constructed cases of tests/golden/rs_cases.py (grid A: block placements; grid B: the
select lines' width, counts, staging passes, policy and the 2^32 border; grid C: select directory and LDS summary; grid D: the block
search of the table kernels).  Per case the index is built once under the case's keys; info() must be what the integer model of the
build says, export() what the reference exported (rs_ref.json; the port where the case passes 2^32 bits); then every query list
runs under every query form the index supports -- the table kernels with 8, 2 and 4 lanes, the rank lines, k_select_lines,
k_select_sdir, k_select_top, k_select_sel, the automatic choice with the sorted hint off and on -- bit-exact against the closed
form over the case's one-positions, and the answers' hashes against the fixture.  A failure names the case, the form, the first
wrong query, what it got and what was expected.  tests/test_rs_host.py keeps the cases and the model honest on the CPU."""
import json
import os

import numpy as np
import pytest

import bitmagic_amd as bm
import rs_cases as rc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U64 = np.uint64
_FX = {}
QUERY_KEYS = {"rs_lanes": 0, "rs_select_lines": 2, "rs_select_top": 0, "rs_select_sel": 0, "rs_sorted_hint": 0}


def fixture():
    if not _FX:
        with open(os.path.join(ROOT, "tests", "golden", "rs_ref.json")) as f:
            _FX.update(json.load(f))
    return _FX["cases"]


def rank_forms(lines):
    k = "k_rank_lines<%d>" if lines else "k_rank_l<%d>"
    return [("k_rank", {"rs_lanes": 8})] + [(k % n, {"rs_lanes": n}) for n in (2, 4)] + \
           [("automatic rank, sorted hint %d" % h, {"rs_sorted_hint": h}) for h in (0, 1)]


def select_forms(c, info):
    f = [("k_select", {"rs_lanes": 8})]
    f += [("k_select_l<%d>" % n, {"rs_lanes": n, "rs_select_lines": 0}) for n in (2, 4)]
    if info["has_lines"]:
        f += [("k_select_lines<%d>" % n, {"rs_lanes": n, "rs_select_lines": 1}) for n in (2, 4)]
        f += [("k_select_sdir<%d>" % n, {"rs_lanes": n}) for n in (2, 4)]
        f += [("k_select_top<%d> (k_select_sdir where the summary was dropped)" % n, {"rs_lanes": n, "rs_select_top": 1}) for n in (2, 4)]
    sel = c.keys["rs_select_sel"]
    if info["select_offset_bits"]:
        f.append(("k_select_sel<u%d>" % info["select_offset_bits"], {"rs_select_sel": sel}))
    f += [("automatic select, sorted hint %d" % h, {"rs_sorted_hint": h, "rs_select_top": -1, "rs_select_sel": sel}) for h in (0, 1)]
    return f


def tune(ctx, keys):
    for k, x in QUERY_KEYS.items(): ctx.set_tuning(k, keys.get(k, x))


def check(c, form, what, q, got, want):
    bad = np.flatnonzero(np.asarray(got) != np.asarray(want))
    if bad.size:
        i = int(bad[0])
        pytest.fail("%r, %s, %s: query %d of %d (= %d): got %d, expected %d (%d wrong)" % (c, form, what, i, len(q), int(q[i]), int(got[i]), int(want[i]), bad.size))


def check_rank(c, v, rs, form, q, want=None):
    """the list back to front first: a kernel that leaves an answer unwritten must not find the right one there from the form before"""
    want = rc.rank_expect(c, q) if want is None else want
    if q.size > 1: check(c, form + ", back to front", "rank", q[::-1], v.rank(q[::-1], rs), want[::-1])
    got = v.rank(q, rs)
    check(c, form, "rank", q, got, want)
    return got


def check_select(c, v, rs, form, r, want=None):
    f, p = rc.select_expect(c, r) if want is None else want
    if r.size > 1:
        found, pos = v.select(r[::-1], rs)
        check(c, form + ", back to front", "select: found", r[::-1], found, f[::-1])
        check(c, form + ", back to front", "select: position", r[::-1], pos, p[::-1])
    found, pos = v.select(r, rs)
    check(c, form, "select: found", r, found, f)
    check(c, form, "select: position", r, pos, p)
    return found, pos


def batch_of(a, n, dead):
    """n queries spread over the list `a`, a dead one among them from four on"""
    b = a[:: max(1, a.size // n)][:n].copy()
    if n >= 4: b[n - 2] = dead
    return b


def run_case(ctx, port, c):
    for k in ("rs_lines", "rs_select_sel", "rs_sdir_shift"): ctx.set_tuning(k, c.keys[k])
    ov = rc.to_oracle(port, c)
    v = bm.bvector.from_block_table(ctx, c.nbits, *ov.flatten())
    rs = v.build_rs_index()
    info = rs.info()
    assert info == rc.expected_info(c), (c, info, rc.expected_info(c))
    for k, x in c.claims.items():
        if k in info: assert info[k] == x, (c, k, info[k], x)
    assert rs.count() == c.count == v.count(), c
    fx = fixture().get(c.name)
    assert (fx is not None) == c.fits_reference(), c
    bc, sub = rs.export()
    if fx:
        assert fx["count"] == c.count and rc.sha(bc, np.uint32) == fx["bcount"] and rc.sha(sub) == fx["sub_count"], (c, "export")
    else:
        pbc, psub = port.rs_build(ov).export(c.nblocks)
        assert (bc[:pbc.size] == pbc).all() and (sub[:psub.size] == psub).all() and not bc[pbc.size:].any() and not sub[psub.size:].any(), (c, "export")
    rank_want, select_want = rc.rank_expect(c, c.rank_q), rc.select_expect(c, c.select_r)      # computed once, shared by the forms
    for i, (form, keys) in enumerate(rank_forms(info["has_lines"])):
        tune(ctx, keys)
        got = check_rank(c, v, rs, form, c.rank_q, rank_want)
        if fx and i == 0:
            assert rc.sha(got[c.rank_q < U64(rc.REF_LIMIT)]) == fx["rank"], (c, "rank answers against the fixture")
        for n in c.batches:
            check_rank(c, v, rs, "%s, batch of %d" % (form, n), batch_of(c.rank_q, n, U64(c.nbits)))
    for i, (form, keys) in enumerate(select_forms(c, info)):
        tune(ctx, keys)
        found, pos = check_select(c, v, rs, form, c.select_r, select_want)
        if fx and i == 0:
            m = c.select_r < U64(rc.REF_LIMIT)
            assert rc.sha(np.concatenate([pos[m], found[m].astype(U64)])) == fx["select"], (c, "select answers against the fixture")
        for n in c.batches:
            check_select(c, v, rs, "%s, batch of %d" % (form, n), batch_of(c.select_r, n, U64(c.count + 1)))
    if c.name.startswith("A."):
        derived(ctx, c, v, rs, fx["derived"])
    del rs, v


def derived(ctx, c, v, rs, fx):
    """count_range, rank_corrected, count_to_test and find_rank over grid A's constructed list, with the table kernels and the automatic choice"""
    d = rc.grid_a_derived(c)
    rk, bit = rc.rank_expect(c, d["pos"]), rc.bit_expect(c, d["pos"])
    ff, fp = rc.find_rank_expect(c, d["rank"], d["from"])
    for form, keys in (("k_rank / k_select", {"rs_lanes": 8}), ("automatic", {"rs_select_sel": c.keys["rs_select_sel"], "rs_select_top": -1})):
        tune(ctx, keys)
        got = v.count_range(d["left"], d["right"], rs)
        check(c, form, "count_range (left)", d["left"], got, rc.count_range_expect(c, d["left"], d["right"]))
        assert rc.sha(got) == fx["count_range"], (c, form)
        got = v.rank_corrected(d["pos"], rs)
        check(c, form, "rank_corrected", d["pos"], got, rk - bit.astype(U64))
        assert rc.sha(got) == fx["rank_corrected"], (c, form)
        got = v.count_to_test(d["pos"], rs)
        check(c, form, "count_to_test", d["pos"], got, np.where(bit, rk, U64(0)))
        assert rc.sha(got) == fx["count_to_test"], (c, form)
        found, pos = v.find_rank(d["rank"], d["from"], rs)
        check(c, form, "find_rank: found (rank)", d["rank"], found, ff)
        check(c, form, "find_rank: position (rank)", d["rank"], pos, fp)
        assert rc.sha(np.concatenate([pos, found.astype(U64)])) == fx["find_rank"], (c, form)


@pytest.mark.parametrize("chunk", list(rc.chunks()))
def test_rank_select_constructed(port, chunk):
    ctx = bm.context(0)
    try:
        for c in rc.chunks()[chunk]():
            run_case(ctx, port, c)
    finally:
        ctx.close()
