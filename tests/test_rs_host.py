"""CPU: the constructed rank / select cases (tests/golden/rs_cases.py) and the reference's answer to them (tests/golden/rs_ref.json,
written by make_rs_golden.py from the reference build).  The fixture is small and holds every case that fits a 32-bit vector; the C
port reproduces it case by case; so do the closed forms over the one-positions, with no oracle at all; the integer model of the
build says what the grids are built to show -- the widths of B1, the policy border of B4, the fb of every C4 row, C3's share of missed
first guesses, the sample shifts of D; where the reference is built the generator reproduces the committed file.
tests/test_gpu_rs.py runs the kernels over the same cases."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import rs_cases as rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
PATH = os.path.join(GOLDEN, "rs_ref.json")
CHUNKS = sorted(rc.chunks())
_FX = {}


def fixture():
    if not _FX:
        with open(PATH) as f:
            _FX.update(json.load(f))
    return _FX["cases"]


def test_fixture_is_small_and_complete():
    assert os.path.getsize(PATH) < 100_000
    fx = fixture()
    want = [c.name for make in rc.chunks().values() for c in make() if c.fits_reference()]
    assert sorted(fx) == sorted(want) and len(set(want)) == len(want)
    left_out = sorted(c.name for make in rc.chunks().values() for c in make() if not c.fits_reference())
    assert left_out == ["B5.far", "B5.straddle", "D.n131073.lines0", "D.n65537.lines0"]          # past 2^32 bits: closed form only
    for name, e in fx.items():
        keys = ["bcount", "count", "rank", "rank_at", "select", "select_at", "sub_count"] + (["derived"] if name.startswith("A.") else [])
        assert sorted(e) == sorted(keys), name
    assert sorted(fx["A.lines0"]["derived"]) == ["count_range", "count_to_test", "find_rank", "rank_corrected"]


@pytest.mark.parametrize("chunk", CHUNKS)
def test_closed_form_matches_reference_fixture(chunk):
    for c in rc.chunks()[chunk]():
        if not c.fits_reference(): continue
        m, e = rc.model_entry(c), fixture()[c.name]
        for k in m:
            assert m[k] == e[k], (c, k, m[k] if not isinstance(m[k], str) else "hash")


@pytest.mark.parametrize("chunk", CHUNKS)
def test_port_matches_reference_fixture(port, chunk):
    for c in rc.chunks()[chunk]():
        if c.fits_reference():
            got, want = rc.oracle_entry(port, c), fixture()[c.name]
            assert got == want, (c, [k for k in want if got[k] != want[k]])
        else:                                                     # past 2^32 bits: the port against the closed form
            rs = port.rs_build(rc.to_oracle(port, c))
            assert (rs.rank(c.rank_q) == rc.rank_expect(c, c.rank_q)).all(), c
            pos, found = rs.select(c.select_r)
            f, p = rc.select_expect(c, c.select_r)
            assert (found == f).all() and (pos[f] == p[f]).all(), c


def test_grid_a_is_what_it_claims(port):
    c = rc.grid_a(0)
    lay = rc.grid_a_layout()
    assert len(lay) == 29 and c.nbits == 29 * rc.B - 777 and int(c.ones[-1]) == c.nbits - 1
    kinds = rc.to_oracle(port, c).flatten()[0].tolist()
    want = {"a": 0, "b": 1, "f": 3, "g": 2, "k": 3, "l": 2}                      # NULL, FULL, GAP, bit-block
    for b, k in enumerate(lay):
        if k in want: assert kinds[b] == want[k], (b, k, kinds[b])
    runs = lambda k: rc.runs_of(rc.class_offsets(k).astype(np.uint64))[0].size
    assert runs("k") == 638 and rc.class_offsets("k")[0] == 0                     # 638 one-runs + 637 zero-runs = 1,275 runs
    assert 2 * runs("g") - 1 > 1275 and rc.class_offsets("f").size == 138 and rc.class_offsets("e").size == 256 and rc.class_offsets("i").size == 8192
    # every class but the last meets two different predecessors, and the running count before it has both parities somewhere
    before = np.searchsorted(c.ones, np.arange(29, dtype=np.uint64) * np.uint64(rc.B))
    assert {int(x) & 1 for x in before} == {0, 1}
    d = rc.grid_a_derived(c)
    assert (d["left"] > d["right"]).any() and (d["from"] >= c.nbits).any() and (d["rank"] == 0).any()
    assert c.rank_q.size == c.nbits + 4 and c.select_r.size == c.count + 3


def test_select_line_widths_follow_the_span_rule():
    """B1: a span of 65,535 keeps 16-bit offsets, 65,536 and a line over a NULL block take 32; B4: the policy's double expression
    switches between 1,920 and 1,921 ones; B5: a line over bit 2^32 keeps 32 bits while it is short, none when it spans 2^32"""
    seen = set()
    for x in rc.B1_X:
        for c in rc.grid_b1(x):
            assert rc.try16(c.nblocks, c.count, 1), c
            assert rc.select_bits(c) == c.claims["select_offset_bits"], c
            K = 60
            first, last = c.ones[::K], c.ones[np.minimum(np.arange(0, c.count, K) + K - 1, c.count - 1)]
            seen.add(int((last - first).max()))
    assert {65535, 65536} <= seen
    for c in rc.grid_b3() + rc.grid_b4() + rc.grid_b5():
        assert rc.select_bits(c) == c.claims["select_offset_bits"], c
    assert [rc.try16(16, n, 1) for n in (1919, 1920, 1921)] == [False, False, True]
    assert not rc.try16(16, 1921, 2)
    s, f = rc.grid_b5()
    assert s.nblocks == f.nblocks == 65538
    line = s.ones[120:150]                                                      # the 30 ones of one 32-bit line
    assert int(line[0]) < (1 << 32) <= int(line[-1]) and int(line[-1] - line[0]) < 6000
    assert int(f.ones[59] - f.ones[30]) >= (1 << 32)
    assert [rc.select_bits(c) for c in rc.grid_b2()] == [32] * 6 + [16] + [32] * 7   # one block: the policy tries 16 bits from 121 ones on


def test_summary_model_claims():
    for c in rc.grid_c4():
        s = rc.Summary(c)
        assert s.spread == c.claims["spread"] and s.fb == c.claims["fb"], (c, s.spread, s.fb)
        assert (s.sdir_shift, s.entries, s.shift, s.n_top) == (6, 66, 6, 66)
    assert [c.nblocks for c in rc.grid_c4()] == [118, 118, 236, 236, 472, 472, 943, 943]
    kept, dropped = [rc.expected_info(c)["bytes"] for c in rc.grid_c4()[-2:]]
    assert kept - dropped == rc.STOP_BYTES == 135168
    c = rc.grid_c3()[0]
    s = rc.Summary(c)
    assert c.nblocks == c.claims["nblocks"] and s.fb == c.claims["fb"]
    r = np.arange(1, c.count + 1, dtype=np.uint64)
    lo, hi, g = s.first_guess(r)
    true_line = rc.line_of(c.ones)[0]
    assert (lo <= true_line).all() and (true_line <= hi).all()
    miss = float((g != true_line).mean())
    print("C3: share of first guesses that miss", miss)
    assert miss >= c.claims["miss_share"]
    for c in rc.grid_c5():
        s = rc.Summary(c)
        assert s.shift == c.claims["stop_shift"] and s.fb == 3 and s.n_top <= rc.STOP_ENTRIES
    assert rc.Summary(rc.grid_c5()[0]).n_top == rc.STOP_ENTRIES
    for c in rc.grid_c2():                                                     # the skewed entry spans the lines it says
        L = int(c.name.split(".")[1][1:])
        lines = rc.line_of(c.ones[::64])[0]
        assert L in np.diff(lines).tolist(), c
    for c in rc.grid_c1():                                                     # the sampled ones stand where the name says
        s = int(c.name.split(".")[1][1:])
        line, bit = rc.line_of(c.ones[:: 1 << s])
        allline = rc.line_of(c.ones)[0]
        if c.name.endswith("first"): assert (bit == 0).all(), c
        if c.name.endswith("last"): assert all((allline == l).sum() == 1 or c.ones[allline == l][-1] == o for l, o in zip(line, c.ones[:: 1 << s])), c
        if c.name.endswith("alone"): assert all((allline == l).sum() == 1 and not np.isin([l - 1, l - 2, l - 3], allline).any() for l in line), c


def test_block_search_cases_sit_on_the_borders():
    shifts = {nb: rc.sample_shape(nb) for nb in rc.D_NBLOCKS}
    assert shifts[2048] == (0, 2048) and shifts[2049] == (1, 1025) and shifts[4096] == (1, 2048) and shifts[4097] == (2, 1025)
    assert shifts[65537] == (6, 1025) and shifts[131073] == (7, 1025) and shifts[16385][0] == 4
    for nb in rc.D_NBLOCKS:
        car = rc.d_carriers(nb)
        sh, ns = shifts[nb]
        G = 1 << sh
        assert car[0] == 0 and car[-1] == nb - 1
        if nb > 16384: assert {16383, 16384} <= set(car)
        if nb >= 2049:
            assert any(b % G == 0 and b for b in car) and any(b % G == G - 1 for b in car), nb
            assert any(b + 41 in car and not any(b < x < b + 41 for x in car) for b in car), nb       # 40 empty blocks between two carriers
        c = rc.d_case(nb, 0)
        assert c.claims["sample_shift"] == sh and c.count == sum(rc.B if i % 3 == 1 else 3 for i in range(len(car)))


def test_generator_reproduces_fixture_where_the_reference_is_built():
    import oracle
    if not oracle.have_reference("avx2"):
        return                                               # (the committed fixture is what the other tests check)
    r = subprocess.run([sys.executable, os.path.join(GOLDEN, "make_rs_golden.py"), "--check"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
