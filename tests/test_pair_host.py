"""CPU: the constructed cases of the pairwise path (tests/golden/pair_cases.py) and the reference's answer to them
(tests/golden/pair_ref.json, written by make_pair_golden.py from the reference build).  The fixture is small and holds the
cells it is for -- every ordered pair of operand kinds, and by name each rare outcome of the storage rule; the C port
reproduces it case by case; so does a NumPy model with no oracle at all (bits from the construction, kinds from
pair_cases.model_kind, a restatement of combine_operation_block_* / clone_assign_block / clone_gap_block); where the
reference is built the generator reproduces the committed file.  tests/test_gpu_pair.py runs the kernels over the same cases."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import pair_cases as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
PATH = os.path.join(GOLDEN, "pair_ref.json")
MODES = ("none", "compress")
_FX = {}


def fixture():
    if not _FX:
        with open(PATH) as f:
            _FX.update(json.load(f))
    return _FX


def _results(name, fl):
    """(op, compress, result kinds per column) of one pair and flavour of the fixture"""
    p = pc.fixture_pairs()[name][0]
    e = fixture()["pairs"][name][pc.flavour_name(fl)]
    for op in pc.OPS:
        for cm, mode in enumerate(MODES):
            yield op, cm, pc.kinds_of_str(e["%s.%s" % (pc.OP_NAMES[op], mode)]["kinds"], p.nblocks)


def test_fixture_is_small_and_complete():
    assert os.path.getsize(PATH) < 100_000
    fx = fixture()
    pairs = pc.fixture_pairs()
    assert sorted(fx["pairs"]) == sorted(pairs) and "long%d" % pc.FIXTURE_N in pairs
    for name, (p, fls) in pairs.items():
        assert sorted(fx["pairs"][name]) == sorted(pc.flavour_name(fl) for fl in fls)
        for fl in fls:
            e = fx["pairs"][name][pc.flavour_name(fl)]
            assert sorted(e) == sorted(["operands"] + ["%s.%s" % (o, m) for o in pc.OP_NAMES for m in MODES])
            assert all(len(s) == (p.n[i] + 1) // 2 for i, s in enumerate(e["operands"]))
    assert sorted(fx["chain"]) == sorted("%s:%s" % c for c in pc.chain_names()) and len(fx["chain"]) == 16
    assert pairs["cut"][0].nbits == 549 * pc.B - 77
    assert len(pc.K_NAMES) == 18 and len(pc.k_columns()) == 324 and len(pc.l_columns()) == 2 * 4 * len(pc.L_LENS) == 224
    assert len(pc.case_columns()) < 2048 <= min(pc.LONG_N)


def test_classes_are_what_they_claim():
    b, runs = pc.class_bits, pc.RUNS
    assert runs["g2_0"] == (2, 0) and runs["g2_1"] == (2, 1) and runs["dfew"] == (3, 0)
    assert 690 <= runs["gA"][0] <= 710 and runs["nA"] == (runs["gA"][0], 1) and (b("nA") == ~b("gA")).all()
    assert not (b("gA") & b("gB")).any() and not (b("gA") | b("gB")).all() and pc.len_sbit(b("gA") | b("gB"))[0] > pc.GAP_RESULT_MAX
    assert not (b("gS") & ~b("gA")).any() and (b("gA") & ~b("gS")).any() and b("gS").any()
    assert runs["g1275_0"] == (1275, 0) and runs["g1275_1"] == (1275, 1) and runs["g1276"] == (1276, 0)
    assert runs["gh"] == (640, 1)
    for x, n in (("gh1", 1275), ("gh2", 1276)):
        assert not (b("gh") & b(x)).any() and pc.len_sbit(b("gh") | b(x))[0] == pc.len_sbit(b("gh") ^ b(x))[0] == n
    assert (b("nd") == ~b("d")).all() and not (b("dS") & ~b("d")).any() and (b("d") & ~b("dS")).any()
    assert abs(int(b("d").sum()) - 32768) < 1000 and runs["d"][0] > 30000
    for ln in pc.L_LENS:
        for sb in (0, 1):
            blk = b("L%d.%d" % (ln, sb))
            g = pc.gap_words(blk).astype(np.int64)
            assert pc.len_sbit(blk) == (ln, sb) and g[1] == 0 and (ln == 2 or g[ln - 1] == pc.B - 2)
            for m in range(8, ln + 1, 8):                   # the one-bit run over every chunk border of the run list
                assert g[m] == g[m - 1] + 1, (ln, m)
    assert {511, 512, 1023, 1024} <= set(pc.L_LENS) and (pc.MAX_GAP_LEN + 8) >> 3 == 160 and (511 + 8) >> 3 == 64 and (512 + 8) >> 3 == 65


def test_grid_l_lengths_as_imported(port):
    """every length of Grid L, both start bits, is the len / start bit of the GAP block the port holds after the import"""
    p = pc.short_pair()
    k, offs, _, gaps = port.import_words(p.words(0, True), True, p.nbits).flatten()
    seen = set()
    for c, (a, _) in enumerate(p.cols):
        if not a.startswith("L"): continue
        assert int(k[c]) == pc.GAP, p.cell(c)
        hdr = int(gaps[int(offs[c])])
        assert (hdr >> 3, hdr & 1) == pc.RUNS[a], p.cell(c)
        g = pc.gap_words(pc.class_bits(a))
        assert (gaps[int(offs[c]):int(offs[c]) + g.size] == g).all(), p.cell(c)
        seen.add((hdr >> 3, hdr & 1))
    assert seen == {(ln, sb) for ln in pc.L_LENS for sb in (0, 1)}


def test_fixture_holds_what_it_is_for():
    fx = fixture()["pairs"]["short"]
    p = pc.short_pair()
    n = p.nblocks
    # every ordered pair of operand kinds
    seen = set()
    for fl in pc.FLAVOURS[:3]:
        ka, kb = [pc.kinds_of_str(s, n) for s in fx[pc.flavour_name(fl)]["operands"]]
        seen |= set(zip(ka.tolist(), kb.tolist()))
    assert seen == {(a, b) for a in range(4) for b in range(4)}
    # the rare outcomes, by name
    found = {k: 0 for k in ("one-run GAP block", "all-zero result stored as BIT", "B | B -> FULL", "GAP x GAP of 1,275 runs -> GAP",
                            "GAP x GAP of 1,276 runs -> GAP", "GAP x GAP of 1,277 runs -> BIT", "computed, compress: 1,275 runs -> GAP",
                            "computed, compress: 1,276 runs -> BIT", "compress: computed -> GAP", "compress: computed -> NULL",
                            "compress: computed -> FULL", "all-ones bit-block against FULL", "all-ones result stored as BIT")}
    for fl in pc.FLAVOURS:
        e = pc.Expect(p, fl)
        ka, kb = [pc.kinds_of_str(s, n) for s in fx[pc.flavour_name(fl)]["operands"]]
        assert (ka == e.kinds[0]).all() and (kb == e.kinds[1]).all(), fl
        gg, bb = (ka == pc.GAP) & (kb == pc.GAP), (ka == pc.BIT) & (kb == pc.BIT)
        none = {}
        for op, cm, kr in _results("short", fl):
            runs, first, pop = e.result(op)[1]
            if not cm:
                none[op] = kr
                found["one-run GAP block"] += int(((kr == pc.GAP) & (runs == 1) & (first == 1)).sum())
                found["all-zero result stored as BIT"] += int(((kr == pc.BIT) & (pop == 0)).sum())
                found["all-ones result stored as BIT"] += int(((kr == pc.BIT) & (pop == pc.B)).sum())
                if op == pc.OR: found["B | B -> FULL"] += int((bb & (kr == pc.FULL)).sum())
                found["GAP x GAP of 1,275 runs -> GAP"] += int((gg & (runs == 1275) & (kr == pc.GAP)).sum())
                found["GAP x GAP of 1,276 runs -> GAP"] += int((gg & (runs == 1276) & (kr == pc.GAP)).sum())
                found["GAP x GAP of 1,277 runs -> BIT"] += int((gg & (runs == 1277) & (kr == pc.BIT)).sum())
                assert not (gg & (runs <= 1276) & (kr == pc.BIT)).any() and not (gg & (runs > 1276) & (kr == pc.GAP)).any(), (fl, op)
                ones_a = (ka == pc.BIT) & (e.facts[0][2] == pc.B) & (kb == pc.FULL)
                found["all-ones bit-block against FULL"] += int(ones_a.sum())
            else:
                computed = (none[op] == pc.BIT) & ~(((ka == pc.BIT) & (kb < pc.BIT)) | ((kb == pc.BIT) & (ka < pc.BIT)))      # (not a copy)
                found["compress: computed -> GAP"] += int((computed & (kr == pc.GAP)).sum())
                found["compress: computed -> NULL"] += int((computed & (kr == pc.NULL)).sum())
                found["compress: computed -> FULL"] += int((computed & (kr == pc.FULL)).sum())
                found["computed, compress: 1,275 runs -> GAP"] += int((bb & (runs == 1275) & (kr == pc.GAP)).sum())
                found["computed, compress: 1,276 runs -> BIT"] += int((bb & (runs == 1276) & (kr == pc.BIT)).sum())
                assert not (bb & (runs >= 1276) & (kr == pc.GAP)).any(), (fl, op)
    print(found)
    assert all(found.values()), found
    # the chain meets blocks no import produces, and copies them
    ch = fixture()["chain"]
    model, first = pc.model_chain()
    r = first["or"]
    assert ((r.k == pc.GAP) & (r.f[0] == 1)).any() and ((r.k == pc.GAP) & (r.f[0] == pc.GAP_RESULT_MAX)).any() and (r.k == pc.FULL).any()
    assert ((first["xor"].k == pc.GAP) & (first["xor"].f[0] == 1)).any()
    copied = pc.kinds_of_str(ch["or:R|0"]["kinds"], n)
    assert (copied[(r.k == pc.GAP) & (r.f[0] == 1)] == pc.FULL).all() and (copied[(r.k == pc.GAP) & (r.f[0] == pc.GAP_RESULT_MAX)] == pc.BIT).all()


@pytest.mark.parametrize("part", ["pairs", "chain"])
def test_port_matches_reference_fixture(port, part):
    """the C port through import_words and op2, as the generator drives the reference"""
    got = _port_fixture(port)[part]
    want = fixture()[part]
    assert sorted(got) == sorted(want)
    for name in want:
        assert got[name] == want[name], (part, name, _where(got[name], want[name]))


_PF = {}


def _port_fixture(port):
    if not _PF:
        _PF.update(pc.oracle_fixture(port))
    return _PF


def _where(got, want, path=""):
    if isinstance(want, dict):
        for k in want:
            w = _where(got[k], want[k], path + "/" + k)
            if w: return w
        return None
    return None if got == want else path


@pytest.mark.parametrize("name", sorted(pc.fixture_pairs()))
def test_model_matches_reference_fixture(name):
    """no oracle at all: words and counts from the construction, kinds from the restated storage rule"""
    p, fls = pc.fixture_pairs()[name]
    for fl in fls:
        e = pc.Expect(p, fl)
        f = fixture()["pairs"][name][pc.flavour_name(fl)]
        for s in (0, 1):
            assert pc.kinds_str(e.kinds[s]) == f["operands"][s], (e, "operand", s, pc.first_diff(e, got_kinds=e.kinds[s], want_kinds=pc.kinds_of_str(f["operands"][s], e.kinds[s].size)))
        for op in pc.OPS:
            for cm, mode in enumerate(MODES):
                m, r = pc.model_entry(e, op, cm), f["%s.%s" % (pc.OP_NAMES[op], mode)]
                assert m["count"] == r["count"] == e.count(op) and m["sha"] == r["sha"], (e, pc.OP_NAMES[op], mode)
                assert m["kinds"] == r["kinds"], (e, pc.OP_NAMES[op], mode, pc.first_diff(e, got_kinds=pc.kinds_of_str(m["kinds"], p.nblocks),
                                                                                       want_kinds=pc.kinds_of_str(r["kinds"], p.nblocks)))


def test_model_matches_reference_fixture_chain():
    model, _ = pc.model_chain()
    p = pc.short_pair()
    e = pc.Expect(p, (True, True))
    for (f, link), lev in model.items():
        r = fixture()["chain"]["%s:%s" % (f, link)]
        assert int(lev.f[2].sum()) == r["count"] and pc.sha(lev.w) == r["sha"], (f, link)
        assert pc.kinds_str(lev.k) == r["kinds"], (f, link, pc.first_diff(e, got_kinds=lev.k, want_kinds=pc.kinds_of_str(r["kinds"], p.nblocks)))


def test_tail_cases_are_on_both_sides_of_their_thresholds():
    for nblocks, ks in pc.SLAB_SPARSE:
        sides = {k: (k * 8 < nblocks * 7 and k > 0) for k in ks}
        assert True in sides.values() and False in sides.values() and all(pc.slab_sparse_mask(nblocks, k).size == k for k in ks)
        lo = max(k for k, s in sides.items() if s)
        assert not sides[lo + 1]                                              # 13 | 14 and 1,791 | 1,792
    assert len(pc.tail_columns(80)) == 80 and pc.tail_columns(81)[-1] == 20 * 1024 and all(c % 1024 < 4 for c in pc.tail_columns(81))
    for op in pc.OPS:
        w = pc.tail_expect(80, op)[1]
        runs = pc.block_facts(w)[0][0]
        assert 1 < runs <= pc.MAX_GAP_LEN                                     # every result column a GAP candidate
    for which in pc.TRIM_CASES:
        p, op = pc.trim_pair(which)
        e = pc.Expect(p, (True, True))
        k = e.result_kinds(op, False)
        assert (e.kinds[0] == pc.GAP).all() and (e.kinds[1] == pc.GAP).all()
        assert int((k == pc.GAP).sum()) == {"none_out": 0, "three_out": 3, "all_out": pc.TRIM_N}[which], which


def test_generator_reproduces_fixture_where_the_reference_is_built():
    import oracle
    if not oracle.have_reference("avx2"):
        return                                               # (the committed fixture is what the other tests check)
    r = subprocess.run([sys.executable, os.path.join(GOLDEN, "make_pair_golden.py"), "--check"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
