"""CPU: the constructed cases of the OR side and of the packed collections (tests/golden/or_cases.py) are what they claim to be.
Every operand uploads, in the oracle port, to the block kinds, run counts and start bits it was built for; the model of the
tile directory (or_cases.tile_record) says of every operand under test what its case claims, and the grids hold every value
they are laid around; the closed form of every case equals the port's agg_or (both optimisation modes), agg_and_sub and
pipeline_counts -- and the reference's on a fixed tenth, where the reference is built; the port reproduces the fixture the
reference wrote (tests/golden/or_ref.json).  The GPU module (tests/test_gpu_or.py) compares the kernels with the same cases."""
import json
import os
import re

import numpy as np
import pytest

import or_cases as oc
import oracle

_PV, _CHECKED = {}, set()
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "bitmagic_amd", "csrc")
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "or_ref.json")


def pvec(orc, v):
    return oc.port_vec(orc, v, _PV)


def kinds_of(e):
    return (e.flatten()[0].tolist() + [0] * oc.NBLOCKS)[:oc.NBLOCKS]


def popcount(w):
    return int(np.unpackbits(w.view(np.uint8)).sum())


def check_operand(port, v):
    """the port holds the vector as built: kinds, header (len, level, start bit) and every run end; an import of the same bits
    gives the same GAP block unless it is one run (then NULL / FULL: why the operands are uploaded as tables)"""
    kinds, offs, _, gaps = pvec(port, v).flatten()
    assert tuple(int(k) for k in kinds) == v.kinds, (v.note, kinds)
    k2, o2, _, g2 = port.import_words(v.words()[:v.nblocks * oc.BW], True, v.nbits).flatten()
    for c, s in enumerate(v.specs):
        if v.kinds[c] != oc.GAP:
            assert int(k2[c]) == v.kinds[c], (v.note, c)
            continue
        assert (gaps[int(offs[c]):int(offs[c]) + s.size] == s).all(), (v.note, c)
        ln, sb = int(s[0]) >> 3, int(s[0]) & 1
        assert (ln, sb) == oc.len_sbit(v.block(c)), (v.note, c)
        if ln == 1: assert int(k2[c]) == (oc.FULL if sb else oc.NULL), (v.note, c)
        else: assert int(k2[c]) == oc.GAP and (g2[int(o2[c]):int(o2[c]) + s.size] == s).all(), (v.note, c)


def test_defines_equal_the_headers():
    """the constants or_cases restates are the ones in the headers (text only: nothing is compiled)"""
    def define(header, name):
        m = re.search(r"^#define\s+%s\s+(\d+)u?\b" % name, open(os.path.join(CSRC, header)).read(), re.M)
        assert m, (header, name)
        return int(m.group(1))
    assert define("bmx_kernels7.h", "ORR_TILE") == oc.ORR_TILE
    assert define("bmx_kernels2.h", "OR_TILE") == oc.OR_TILE
    assert define("bmx_kernels10.h", "C2_GROUP") == oc.C2_GROUP
    assert define("bmx_kernels8.h", "CM_WAVES") == oc.CM_WAVES
    assert define("bmx_kernels2.h", "DIRECT_MAX_OPS") == oc.DIRECT_MAX_OPS


def test_fillers(port):
    f = oc.fillers()
    assert len(f) == oc.N_FILLERS == 63
    for v in f:
        check_operand(port, v)
        for t in range(3):
            r = oc.tile_record(v, t)
            assert not r["slow"] and not r["long"] and r["nch"] == (14, 14, 3)[t] and r["single"][:3] == [3, 3, 3]
    assert (oc.union_words(f) == oc.filler_union()).all()                       # the closed form of the filler union
    assert (oc.union_words(f[:5] + f[6:]) == oc.filler_union([i for i in range(63) if i != 5])).all()
    assert popcount(oc.filler_union()) == 63 * 3 * oc.NBLOCKS
    gw, gb = map(sum, zip(*[v.gap_stats() for v in f]))
    assert oc.rows_wanted(gw, gb)                                               # sparse enough for the row kernel by default


def test_words_equal_the_plain_decode():
    """Vec.words() builds the bits from the run lists; the plain decode of every block (block_of_ends) gives the same words, and
    gap_of() the GAP words gap_words(block_of()) gives -- over the operands under test and a third of the collections' members"""
    for runs, bits in (((), ()), ([(0, 5)], [9]), ([(3, 9), (100, oc.B - 1)], [50]), ((), [0, oc.B - 1]), ([(0, oc.B - 1)], ())):
        assert (oc.gap_of(runs, bits) == oc.gap_words(oc.block_of(runs, bits))).all(), (runs, bits)
    vs = {o.uid: o for g in oc.N_CASES for c in oc.grid(g) for o in c.ops}
    for name in ("bags", "fold", "dir"):
        for m in oc.coll(name).members[::3]: vs[m.uid] = m; vs[m.complement().uid] = m.complement()
    for v in vs.values():
        assert (v.words() == v.words_plain()).all(), v.note


def test_model_of_the_tile_directory():
    """tile_record on hand-made tiles: the pair model counts the runs the bits hold, also where the fourth pair of a block's last
    chunk reaches into the next block's header ((len + 1) % 8 == 0: the block's last word, 0xFFFF, reads as "no run")"""
    for ln in list(range(2, 40)) + [63, 64, 65]:
        t = {k: oc.block_with_len(ln + k % 3, 0) for k in range(oc.ORR_TILE)}
        x = oc.xvec(t)
        r = oc.tile_record(x, 1)
        if r["slow"]:
            assert r["nch"] > 64 and r["why"] == ("chunks",) and r["M"] == 0
            continue
        starts = np.cumsum([0] + r["ch"][:-1])
        assert r["M"] == sum(1 << int(s) for s in starts if s < 64)
        for k in range(oc.ORR_TILE):
            assert (r["multi"][k], r["single"][k]) == oc.run_counts(x.block(oc.ORR_TILE + k)), (ln, k)
    assert [oc.nth_set_bit16(0x2AAA, r) for r in range(7)] == [1, 3, 5, 7, 9, 11, 13]
    for nm in range(10):
        for ns in range(18):
            L = oc.bag_layout(nm, ns)
            assert L["singles_at"] % 4 == 0 and L["singles_at"] - nm == L["pad_m"] < 4 and L["words"] == L["singles_at"] + (ns + L["pad_s"]) // 2


def test_grids_cover_what_they_name():
    """every value listed under the grids occurs, and the model says so"""
    o1 = oc.grid("O1")
    P = lambda key: [c.params[key] for c in o1 if key in c.params]
    # O1: len at every residue mod 8 at one, two and three chunks and next to the longest GAP block; both start bits; the columns
    lens = {(c.params["len"], c.params["sbit"]) for c in o1 if "len" in c.params}
    for lo in (1, 8, 16, oc.MAX_GAP_LEN - 7):
        assert all((ln, sb) in lens for ln in range(lo, lo + 8) for sb in (0, 1) if (ln, sb) != (1, 1)), lo
    assert {(ln + 8) >> 3 for ln, _ in lens if ln < 100} >= {1, 2, 3}
    for ln in (7, 8, 15, 16, 23, 24):
        assert {c.params["col"] for c in o1 if c.params.get("len") == ln} == set(oc.O1_COLS)
    for c in o1:
        r = oc.tile_record(c.x, 1)
        if c.x.nblocks > oc.ORR_TILE: assert r["first"] == oc.ORR_TILE                 # behind tile 0's data: a non-zero first chunk
        if c.params.get("sbit") == 1: assert r["slow"] and "sbit" in r["why"], c     # start bit 1 makes the tile slow
        t0 = oc.tile_record(c.x, 0)
        assert t0["long"] and not t0["slow"] and t0["nch"] == 14, c                 # the decoys
    # tile totals
    assert {(c.params["total"], c.params["longpos"]) for c in o1 if "longpos" in c.params} == {(t, p) for t in (63, 64, 65) for p in (0, 13)}
    for c in o1:
        r = oc.tile_record(c.x, 1)
        if c.params.get("total") == 65: assert r["slow"] and r["why"] == ("chunks",)
        if c.params.get("total") == 64: assert not r["slow"] and r["nch"] == oc.ROW_CHUNKS and 0 < r["M"] < (1 << 64)     # lane 63 holds the last chunk
        if "lastlen" in c.params:
            assert (63, 2) in r["multi_pairs"] and (63, 3) not in r["multi_pairs"] and r["ch"][13] == 4, c
            g = c.x.specs[oc.ORR_TILE + 13]
            assert (g.size % 8 == 0) == (c.params["lastlen"] == 31)                 # len 31: word 7 of chunk 63 is the block's last word
    # masks: every position of nth_set_bit16
    assert set(P("mask")) == set(oc.O1_MASKS)
    for p in range(oc.ORR_TILE):
        m = oc.O1_MASKS["allbut%d" % p]
        assert [oc.nth_set_bit16(m, r) for r in range(13)] == [k for k in range(14) if k != p]
    assert {(c.params["full"], c.params["fullwith"]) for c in o1 if "full" in c.params} == {(k, w) for k in oc.O1_COLS for w in (0, 1)}
    for c in o1:
        if "full" in c.params:
            col = oc.ORR_TILE + c.params["full"]
            w, _, k0, k1 = c.expect()
            assert k0[col] == k1[col] == oc.FULL and (w[col * oc.BW:(col + 1) * oc.BW] == 0xFFFFFFFF).all()
            if c.params["fullwith"]: assert any(o.kind(col) == oc.GAP and o.uid != c.x.uid and o.note.startswith("o1.") for o in c.ops)
    nb = set(P("nblocks_"))
    assert nb == set(oc.O1_NBLOCKS) and 14 in nb and 28 in nb and any(14 < n < 28 for n in nb)
    assert set(P("long")) == {"clear", "pair0", "pair3", "lastchunk"}
    for c in o1:
        if "long" in c.params:
            r = oc.tile_record(c.x, 1)
            assert sum(r["multi"]) == (0 if c.params["long"] == "clear" else 1), c
    assert set(P("shape")) == set(oc.SHAPES) | set(oc.ENDS) | {"shared"}
    for name, (ln, sb) in oc.ENDS.items():
        b = oc.block_with_len(ln, sb)
        assert bool(b[-1]) == name.startswith("end1") and (ln + 1) % 8 == (0 if name.endswith("r0") else 1)
    c = [c for c in o1 if c.params.get("shape") == "shared"][0]
    col = oc.ORR_TILE + 7
    both = c.x.block(col) & np.unpackbits(oc.filler_union()[col * oc.BW:(col + 1) * oc.BW].view(np.uint8), bitorder="little").astype(bool)
    assert both.any()                                                            # the run covers a filler's bit
    # O2
    o2 = oc.grid("O2")
    plain = [c for c in o2 if not c.params["nulls"] and not c.params["second"]]
    assert {c.params["n"] for c in plain} == set(oc.O2_N)
    for n in oc.O2_N:
        assert {c.params["idx"] for c in plain if c.params["n"] == n} == {i for i in oc.O2_IDX if i < n} | {n - 1}
    assert {(c.params["nulls"], c.params["where"]) for c in o2 if c.params["nulls"]} == {(k, w) for k in (1, 2, 3) for w in ("before", "between", "after")}
    assert {c.params["second"] for c in o2} == {None, "batch", "next"}
    for c in o2:
        assert len(c.ops) == c.params["n"] and c.ops[c.params["idx"]] is c.x
        ix = [i for i, o in enumerate(c.ops) if o.note == "o2.x2"]
        if c.params["second"]:                                                   # same wave; the same batch of 1,024 or the next one
            d = ix[0] - c.params["idx"]
            assert d % oc.ROW_WAVES == 0 and d // (oc.ROW_WAVES * oc.ROW_BATCH) == (1 if c.params["second"] == "next" else 0)
        assert sum(1 for o in c.ops if not any(k == oc.GAP for k in o.kinds)) == c.params["nulls"]
    # O3: bags
    bags = oc.coll("bags")
    tot = [bags.totals(c) for c in range(oc.NBLOCKS)]
    assert tot == list(zip(oc.O3_NM, oc.O3_NS))
    assert {m % 4 for m, s in tot} == set(range(4)) and {s % 8 for m, s in tot} == set(range(8))
    assert {m for m, s in tot} == set(range(10)) and {s for m, s in tot} == set(range(18))
    assert (0, 0) in tot and any(m == 0 and s for m, s in tot) and any(s == 0 and m for m, s in tot)
    assert {oc.bag_layout(m, s)["pad_m"] for m, s in tot} == set(range(4)) and {oc.bag_layout(m, s)["pad_s"] for m, s in tot} == set(range(8))
    assert any(v.kind(30) == oc.FULL for v in bags.members)
    # O3: the fold
    fold = oc.coll("fold")
    F = oc.FOLD_COLS
    assert 40 % oc.fold_w(256) == 0 and 44 % oc.fold_w(512) == 0 and 44 % oc.fold_w(256) != 0
    assert 256 == 64 * oc.fold_w(512) and 512 == 64 * oc.fold_w(256)
    for b in oc.FOLD_BOUNDS:
        runs = oc.fold_runs(b)
        assert {oc.interior(r)[0] for what, d, r in runs if what == "first"} == {b - 1, b, b + 1}
        assert {oc.interior(r)[1] for what, d, r in runs if what == "last"} == {b - 1, b, b + 1}
        for j, (_, _, r) in enumerate(runs):
            assert (fold.members[10 + j].block(F["b%d" % b]) == oc.block_of([r])).all()
    assert fold.members[16].block(F["w2047"])[-1] and oc.interior((32 * 2040 + 5, oc.B - 1)) == (2041, 2046)
    for tag, m in (("stack2", 2), ("stack3", 3), ("stack64", 64)):
        assert sum(1 for v in fold.members if v.kind(F[tag]) == oc.GAP and v.block(F[tag])[32 * 105]) == m
    a, b = oc.interior((32 * 200 + 5, 32 * 203 + 4)), oc.interior((32 * 202 + 9, 32 * 206 + 1))
    assert a[1] + 1 == b[0]                                                      # interiors abut without overlap
    assert oc.bag_round_entries(512) < fold.totals(F["multis1"])[0] <= 2 * oc.bag_round_entries(512) < fold.totals(F["multis2"])[0]
    assert fold.totals(F["singles1"])[1] > oc.singles_round(512)
    assert len(fold.counts(F["multis1"])) >= 64 and max(m for m, s in fold.counts(F["multis1"])) == oc.HEAVY_RUNS
    why = set()
    for v in fold.members:
        for t in range(3): why |= set(oc.tile_record(v, t)["why"]) or {"fast"}
    assert why == {"chunks", "full", "sbit", "fast"}
    assert fold.members[33].block(F["edges"])[0] and fold.members[34].block(F["edges"])[-1]      # runs [0, x] and [x, 65535]
    # O4: pieces of 0, 1, 15, 16, 17, 32, 33 entries, multi-bit and single-bit independently
    d = oc.coll("dir")
    seen = set()
    for c in range(oc.NBLOCKS):
        k = d.counts(c)
        for j in range(7):
            assert k[oc.O4_T0 + j] == oc.o4_piece(j, c)
            seen.add(k[oc.O4_T0 + j])
    assert seen == {(a, b) for a in oc.O4_COUNTS for b in oc.O4_COUNTS}
    ls = oc.o4_lists()
    assert {m for m, p, t, o, l in ls if o == "asis"} == set(oc.O4_M)
    assert {p for m, p, t, o, l in ls if o == "asis"} == set(oc.O4_POS) and {o for m, p, t, o, l in ls} == {"asis", "reverse", "repeats"}
    for m, p, t, o, l in ls:
        assert len(l) == m and l[p] == oc.O4_T0 + t and (len(set(l)) == m) == (o != "repeats")
    assert [len(g) for g in oc.o4_pipelines()] == list(oc.O4_GROUPS)
    assert oc.coll("short").members[0].nblocks < oc.NBLOCKS
    assert {oc.coll(n).n for n in oc.COLLS_DIR[1:]} == set(oc.O4_SIZES) and {oc.coll("bags%d" % n).n for n in oc.O5_SIZES} == set(oc.O5_SIZES)
    assert set(oc.o6_residues()) == set(range(8))                                # O6: every (len + 1) % 8, a NULL and a FULL column in tile 1
    blocks = oc.o6_pattern()[0]
    assert not blocks[oc.ORR_TILE + 12].any() and blocks[oc.ORR_TILE + 13].all() and all(oc.kind_of(b) == oc.GAP for b in blocks[:oc.ORR_TILE + 12])
    print("cases per grid:", {g: len(oc.grid(g)) for g in oc.N_CASES}, "lists O4:", len(ls))


FULLVEC = []


def fullvec():
    if not FULLVEC: FULLVEC.append(oc.Vec(["full"] * oc.NBLOCKS, note="all ones"))
    return FULLVEC[0]


def check_case(orc, c, operands_too):
    if operands_too:
        for o in {o.uid: o for o in c.ops if not o.note.startswith("filler")}.values():
            if o.uid not in _CHECKED: check_operand(orc, o)
            _CHECKED.add(o.uid)
        r = oc.tile_record(c.x, 1)
        for key, want in c.claims.items():
            if want is not None and key in r: assert r[key] == want, (c, key, r[key], want)
        assert len(c.ops) >= oc.N_ROWS and all(oc.BIT not in o.kinds for o in c.ops), c
    w, cnt, k0, k1 = c.expect()
    pv = [pvec(orc, o) for o in c.ops]
    for opt, kk in ((False, k0), (True, k1)):
        e = orc.agg_or(pv, opt)
        assert (e.to_words(oc.NW) == w).all(), (c, opt)
        assert e.count() == cnt and kinds_of(e) == kk, (c, opt, kinds_of(e), kk)
    if not orc.is_ref:
        # the same list in the AND role (complements) and as a SUB list: the complement of the union
        pa = [pvec(orc, o.complement()) for o in c.ops if o.nblocks == oc.NBLOCKS]
        short = [o for o in c.ops if o.nblocks < oc.NBLOCKS]
        inv = ~oc.union_words([o for o in c.ops if o.nblocks == oc.NBLOCKS])
        assert (orc.agg_and_sub(pa, [pvec(orc, o) for o in short]).to_words(oc.NW) == ~w).all(), c
        assert (orc.agg_and_sub([pvec(orc, fullvec())], pv).to_words(oc.NW) == ~w).all(), c
        got = orc.pipeline_counts([(pa, []), ([pvec(orc, fullvec())], pv)])
        assert [int(x) for x in got] == [popcount(inv), oc.NBITS - cnt], c


@pytest.mark.parametrize("grid,k", oc.chunks())
def test_closed_form_equals_the_oracle(port, grid, k):
    for c in oc.chunk(grid, k):
        check_case(port, c, True)


def check_coll(orc, name):
    C = oc.coll(name)
    nb = C.members[0].nblocks
    u = C.union()
    pv = [pvec(orc, m) for m in C.members]
    for opt in (False, True):
        e = orc.agg_or(pv, opt)
        assert (e.to_words(oc.NW) == u).all() and kinds_of(e) == oc.kinds_of_union(u, C.members, opt), (name, opt)
    if orc.is_ref: return
    for m in C.members: check_operand(orc, m)
    inv = ~u
    inv[nb * oc.BW:] = 0
    pa = [pvec(orc, m) for m in C.vecs("and")]
    assert (orc.agg_and_sub(pa, []).to_words(oc.NW) == inv).all(), name
    assert int(orc.pipeline_counts([(pa, [])])[0]) == popcount(inv), name


@pytest.mark.parametrize("name", oc.COLLS_FULL + oc.COLLS_DIR + ("short",))
def test_collections_equal_the_oracle(port, name):
    check_coll(port, name)


def test_member_lists_and_pipelines_equal_the_oracle(port):
    """O4: the union / intersection of every member list, the counts of every pipeline (AND lists from the AND-role vectors, SUB
    lists from the OR-role ones -- also from the shorter collection), as NumPy computes them from the members' words"""
    C, S = oc.coll("dir"), oc.coll("short")
    w, wa = C.words(), C.words("and")
    pv, pa = [pvec(port, m) for m in C.members], [pvec(port, m) for m in C.vecs("and")]
    for m, p, t, o, l in oc.o4_lists():
        assert (port.agg_or([pv[i] for i in l]).to_words(oc.NW) == C.union(l)).all(), (m, p, o)
        assert (port.agg_and_sub([pa[i] for i in l], []).to_words(oc.NW) == np.bitwise_and.reduce(wa[sorted(set(l))], axis=0)).all(), (m, p, o)
    ps = [pvec(port, m) for m in S.members]
    for groups in oc.o4_pipelines():
        want = [popcount(np.bitwise_and.reduce(wa[sorted(set(a))], axis=0) & ~np.bitwise_or.reduce(w[sorted(set(s))], axis=0)) for a, s in groups]
        assert [int(x) for x in port.pipeline_counts([([pa[i] for i in a], [pv[i] for i in s]) for a, s in groups])] == want
        short = [popcount(np.bitwise_and.reduce(wa[sorted(set(a))], axis=0) & ~S.union([i % S.n for i in s])) for a, s in groups]
        assert [int(x) for x in port.pipeline_counts([([pa[i] for i in a], [ps[i % S.n] for i in s]) for a, s in groups])] == short


@pytest.mark.skipif(not oracle.have_reference("avx2"), reason="needs the reference build (oracle/_ref)")
def test_closed_form_equals_the_reference_on_a_tenth():
    ref = oracle.reference("avx2")
    n = 0
    for g in oc.N_CASES:
        for c in oc.grid(g)[3::10]:
            check_case(ref, c, False)
            n += 1
    for name in oc.COLLS_FULL:
        check_coll(ref, name)
    assert n >= 28


def test_port_reproduces_the_fixture(port):
    """tests/golden/or_ref.json was written by the reference; the port computes the same kinds, counts and hashes"""
    with open(FIXTURE) as f:
        fx = json.load(f)
    assert oc.oracle_fixture(port, _PV)["cases"] == fx["cases"]
    assert len(fx["cases"]) == len(oc.recorded()) and os.path.getsize(FIXTURE) <= os.path.getsize(os.path.join(os.path.dirname(FIXTURE), "rs_ref.json"))


@pytest.mark.skipif(not oracle.have_reference("avx2"), reason="needs the reference build (oracle/_ref)")
def test_generator_reproduces_the_fixture():
    import make_or_golden
    assert make_or_golden.generate() == open(FIXTURE).read()
