"""CPU: the constructed cases of the id-list import (tests/golden/ids_cases.py) are what they claim to be.  The constants the
module restates are the ones in the headers and bmx.hip; plan() says of every case that it meets the border its name claims;
the closed form expected_table() equals the oracle port's set_bit-per-id table for every case of at most PORT_LIMIT ids (and for
a shrunken twin of each larger one), the committed import_ref.json for its 14 lists, and the reference itself on the recorded
subset (tests/golden/ids_ref.json); the window tables of a partition concatenate to the single table.  The GPU module
(tests/test_gpu_ids.py) compares the kernels with the same cases."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import ids_cases as ic
import import_cases
import oracle
from and_fold_cases import len_sbit

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "bitmagic_amd", "csrc")
GOLDEN = os.path.join(ROOT, "tests", "golden")
FIXTURE = os.path.join(GOLDEN, "ids_ref.json")
B = ic.B


def test_constants_equal_the_source():
    """the constants ids_cases restates are the ones in the source (text only: nothing is compiled)"""
    def text(name): return open(os.path.join(CSRC, name)).read()
    def define(header, name):
        m = re.search(r"^#define\s+%s\s+(\d+)u?\b" % name, text(header), re.M)
        assert m, (header, name)
        return int(m.group(1))
    assert define("bmx_kernels13.h", "IDS_CHUNK") == ic.IDS_CHUNK
    assert define("bmx_kernels13.h", "TBL_PER") == ic.TBL_PER
    assert define("bmx_kernels13.h", "IDS_LDS_BLOCKS") == ic.IDS_LDS_BLOCKS
    assert define("bmx_kernels.h", "SCAN_LAYOUT_PER") == ic.SCAN_LAYOUT_PER
    k13, k0, hip = text("bmx_kernels13.h"), text("bmx_kernels.h"), text("bmx.hip")
    assert "k0 < end; k0 += %du" % ic.IMAGE_BATCH in k13                                        # ids_image
    assert "runs < %du ? (u32)K_GAP" % ic.GAP_RUNS_END in k13 and ic.GAP_RUNS_END == ic.MAX_GAP_LEN + 1
    assert "len <= 124u ? 0u : len <= 252u ? 1u : len <= 508u ? 2u : 3u" in k13                  # gap_close: the level borders
    assert "base += 1024u * SCAN_LAYOUT_PER" in k0 and "w * (64u * SCAN_LAYOUT_PER)" in k0
    assert "(n + %d) / %d, %du)" % (ic.LGRID_IDS - 1, ic.LGRID_IDS, ic.LGRID_MAX) in hip       # lgrid
    assert "const u64 per = (n + lgrid - 1) / lgrid;" in hip and "const bool lds = nbl <= IDS_LDS_BLOCKS;" in hip
    assert "const size_t lds_b = (size_t)nbl * 4;" in hip
    assert "(nchunks + TBL_PER - 1) / TBL_PER" in hip and "(nbl + TBL_PER - 1) / TBL_PER" in hip
    assert "#define IDS_MAX_BLOCKS (65536u * 16u)" in hip and ic.IDS_MAX_BLOCKS == 65536 * 16


def test_module_imports_quickly_and_counts_hold():
    r = subprocess.run([sys.executable, "-c", "import sys, time; sys.path.insert(0, %r); t = time.perf_counter(); import ids_cases; "
                        "print(time.perf_counter() - t)" % GOLDEN], capture_output=True, text=True, check=True)
    assert float(r.stdout) < 2.0
    assert {g: len(ic.grid(g)) for g in ic.N_CASES} == ic.N_CASES
    assert 2 <= len(ic.BIG) <= 6 and all(n.startswith(("I1/two_parts", "I2/wg512")) for n in ic.BIG)
    print("cases per grid:", ic.N_CASES, "large:", ic.BIG)


def _block(c, blk=1):
    b = np.zeros(B, bool); b[ic.block_offsets(c.spec)[blk]] = True
    return b


def test_every_case_meets_the_border_it_names():
    seen = {"descent": set(), "change": set(), "lds": set(), "nparts": set(), "per": set(), "residue": set(), "level": set()}
    for c in ic.CASES.values():
        ids = c.ids()
        p = ic.plan(ids, c.nbits)
        q = c.claims
        assert p["n"] == c.n and p["size"] == c.size(), c
        assert p["sorted"] == c.sorted, c                                  # the order decides the path, never the flag
        if "n" in q: assert p["n"] == q["n"]
        if "change" in q:
            assert q["change"] in p["changes"], c
            if c.name.startswith("I1/change_at"): assert p["changes"].tolist() == [q["change"]]
            seen["change"].add((q["change"] % ic.IDS_CHUNK == 0, q["change"] % 256 == 0, q["change"] % 64 == 0))
        if q.get("cap_is_n"): assert p["cap"] == p["n"] == ic.IDS_CHUNK + 1 and p["touched"] == p["n"]
        if "zero_start_chunks" in q:
            assert int((p["chunk_starts"] == 0).sum()) == q["zero_start_chunks"] and ic.block_offsets(c.spec)[3].size < 70000 == spec_ids(c, 3)
        if c.name == "I1/last_chunk_one_id":
            assert p["n"] % ic.IDS_CHUNK == 1 and p["changes"].tolist() == [p["n"] - 1] and p["chunk_starts"][-1] == 1
        for i in q.get("equal_at", ()):
            assert ids[i] == ids[i - 1] and i % ic.IDS_CHUNK == 0, (c, i)
        if "nparts" in q:
            assert p["nparts"] == q["nparts"] and p["sorted"], c
            assert set(q["change_chunks"]) <= set((p["changes"] // ic.IDS_CHUNK).tolist()), c
            if q["nparts"] == 2:
                assert p["chunk_starts"][ic.TBL_PER] >= 1 and p["chunk_starts"][-1] >= 1 and p["chunk_starts"][ic.TBL_PER - 1] >= 1
            else: assert p["nchunks"] == ic.TBL_PER                                  # the last size one workgroup scans
            seen["nparts"].add((q["nparts"], p["nchunks"]))
        if "descent" in q:
            assert p["descents"].tolist() == [q["descent"]] and p["block_runs"] > p["distinct_blocks"], c
            seen["descent"].add(q["descent"])
        if "lgrid" in q:
            assert (p["lgrid"], p["per"]) == (q["lgrid"], q["per"]) and p["lds"], c
            dup = np.uint64(3 * B + B - 1)
            for g in range(p["lgrid"]):                                              # block 3 and the duplicated id in every workgroup
                part = ids[g * p["per"]:(g + 1) * p["per"]]
                assert part.size and (part == dup).sum() == 2 and ((part >> np.uint64(16)) == 3).sum() == 62, (c, g)
            seen["per"].add(p["per"])
        if "nbl" in q:
            assert p["nbl"] == q["nbl"] and p["lds"] == q["lds"] and p["lds_bytes"] == q["nbl"] * 4 and not p["sorted"], c
            touched = set(ic.block_offsets(c.spec))
            assert touched == {0, 4095, 4096, 4097, 8191, 8192, 8193, q["nbl"] - 1} and p["nparts"] == (q["nbl"] + 4095) // 4096 >= 4
            seen["lds"].add((p["lds"], p["lds_bytes"]))
        if c.grid == "I2" and c.order in ("rev", "perm"):
            assert p["lgrid"] == min(-(-p["n"] // 4096), 512) and p["per"] == -(-p["n"] // p["lgrid"])
            seen["per"].add(p["per"])
        if c.grid == "I3":
            assert p["touched"] == 1 and p["distinct_blocks"] == 1
            b = _block(c)
            if "ids" in q: assert p["n"] == q["ids"]
            if "runs" in q:
                assert len_sbit(b) == (q["runs"], q["first"]) and bool(b[-1]) == bool(q["first"] ^ ((q["runs"] - 1) & 1)), c
                assert int(c.expected(True)[1][1]) == (ic.GAP if q["runs"] <= ic.MAX_GAP_LEN else ic.BIT)
                seen["residue"].add(((q["runs"] + 1) % 8, q["first"])); seen["level"].add(q["runs"])
            if "bits" in q: assert np.flatnonzero(b).tolist() == sorted(q["bits"]), c
            for pos in q.get("ends", ()): assert b[pos] and (pos == B - 1 or not b[pos + 1]) and b.sum() == min(pos, 40) + 1
            for pos in q.get("starts", ()): assert b[pos] and (pos == 0 or not b[pos - 1]) and b.sum() == min(B - pos, 41)
        if c.grid == "I4":
            T = q["touched"]
            assert p["touched"] == T and (p["sorted"] or p["lds"])
            k1 = c.expected(True)[1]; k0 = c.expected(False)[1]
            t1 = k1[k1 != 0]
            assert t1.size == T and (k0[k0 != 0] == ic.BIT).all() and (k1 == 0).sum() >= T // 4         # untouched blocks between them
            assert set(t1.tolist()) == {ic.FULL, ic.GAP, ic.BIT}
            assert [int(k) for k in t1] == [ic.i4_kind(T, t) for t in range(T)]
            if T >= ic.LAYOUT_PASS - 1:      # every lane and every step of a wave of k_scan_layout meets a bit-block and a GAP block
                for kind in (ic.BIT, ic.GAP):
                    t = np.flatnonzero(t1 == kind)
                    assert set((t % 64).tolist()) == set(range(64)) and set((t % ic.LAYOUT_WAVE // 64).tolist()) == set(range(ic.SCAN_LAYOUT_PER))
                assert t1[T // 2] == ic.FULL and t1[T - 2] == ic.FULL                    # a FULL block inside pass 0 and next to its end
        if "size" in q: assert p["size"] == q["size"]
    assert seen["descent"] == set(ic.DESCENT_AT)
    assert {(True, True, True), (False, True, True), (False, False, True), (False, False, False)} <= seen["change"]
    assert seen["lds"] == {(True, 65532), (True, 65536), (False, 65540)}
    assert seen["nparts"] == {(1, 4096), (2, 4097), (2, 4098)}
    assert {4095, 4096, 4097, 2049} <= seen["per"]                                       # n = 4,096 k +- 1, and the 512 cap
    assert seen["residue"] >= {(r, f) for r in range(8) for f in (0, 1)} and seen["level"] >= set(ic.LEVEL_LENS)
    assert {c.claims["touched"] for c in ic.grid("I4")} == {w + d for w in (4, 64, ic.LAYOUT_WAVE, ic.LAYOUT_PASS) for d in (-1, 0, 1)}
    assert {c.claims["ids"] for c in ic.grid("I3") if "ids" in c.claims} >= {ic.IMAGE_BATCH + d for d in (-1, 0, 1)} | {B, B + 70}
    w4 = ic.CASES["I6/w4_high"].ids()
    assert w4.min() == (1 << 31) - 1 and w4.max() == (1 << 32) - 1 and (w4.astype(np.uint32).view(np.int32) < 0).sum() == 3
    assert ic.CASES["I6/w8_high"].widths() == (8,) and ic.CASES["I6/w8_high"].size() == 1 << 36


def spec_ids(c, blk):
    return sum(o.size * r for b, o, r in c.spec if b == blk)


_PORT_DONE = {}


def _port_check(port, c):
    """oracle_table (set_bit per id, optimize() when asked) against the closed form; once per list content"""
    key = (id(c.spec), c.nbits)
    if key in _PORT_DONE: return 0
    ids = c.ids()
    for opt in (False, True):
        nbits_out, table, count = import_cases.oracle_table(port, ids, c.nbits, opt)
        e = c.expected(opt)
        assert nbits_out == e[0] == c.size() and count == c.uniq().size, c
        assert ic.record(*table) == ic.record(*e[1:]), (c, opt)
    _PORT_DONE[key] = True
    return 1


@pytest.mark.parametrize("grid", sorted(ic.N_CASES))
def test_closed_form_equals_the_oracle_port(port, grid):
    small = [c for c in ic.grid(grid) if c.n <= ic.PORT_LIMIT]
    big = [c for c in ic.grid(grid) if c.n > ic.PORT_LIMIT]
    assert len(small) + len(big) == ic.N_CASES[grid] and sorted(c.name for c in big) == [n for n in ic.BIG if n.startswith(grid)]
    for c in small: _port_check(port, c)
    twins = 0
    for c in big:
        t = c.shrunk()
        assert t.n <= ic.PORT_LIMIT and [(b, o.tolist()) for b, o, _ in t.spec] == [(b, o.tolist()) for b, o, _ in c.spec]
        assert _port_check(port, t) == 1
        for opt in (False, True):                                                 # the same union: the same table but for the size
            assert all((a == b).all() for a, b in zip(t.expected(opt)[1:], c.expected(opt)[1:]))
        twins += 1
    assert twins == len(big)


def test_closed_form_equals_the_committed_import_fixture():
    """the 14 lists of import_ref.json, which the reference wrote: the model gives the same records"""
    with open(os.path.join(GOLDEN, "import_ref.json")) as f:
        fx = json.load(f)["cases"]
    lists = import_cases.cases()
    assert sorted(fx) == sorted(lists) and len(fx) == 14
    for name, (ids, nbits, _) in lists.items():
        spec = ic.spec_from_ids(ids)
        assert (ic.expand(spec) == ids).all()
        for opt in (0, 1):
            e = ic.expected_table(spec, nbits, bool(opt))
            assert e[0] == fx[name]["nbits_out"] and ic.record(*e[1:]) == fx[name]["opt%d" % opt], (name, opt)


def test_fixture_port_and_closed_form_agree(port):
    with open(FIXTURE) as f:
        fx = json.load(f)["cases"]
    rec = ic.recorded()
    assert os.path.getsize(FIXTURE) < 100_000 and sorted(fx) == sorted(c.name for c in rec)
    names = {c.name for c in rec}
    assert {c.name for c in ic.grid("I6")} <= names
    assert {"I3/s/runs_%d_first_%d" % (ln, s) for ln in ic.LEVEL_LENS for s in (0, 1)} <= names
    for g in ("I1", "I4"):
        assert len([n for n in names if n.startswith(g)]) >= (ic.N_CASES[g] - 3) // 4
    assert {fx[c.name]["flavour"] for c in rec if c.max_id() >= (1 << 32)} == {"avx2_64"}
    for c in rec:
        r = fx[c.name]
        ids = c.ids()
        assert r["n"] == c.n and r["nbits"] == c.nbits and r["nbits_out"] == c.size() and r["count"] == c.uniq().size
        for opt in (0, 1):
            assert ic.record(*c.expected(bool(opt))[1:]) == r["opt%d" % opt], (c, opt)
            nbits_out, table, count = import_cases.oracle_table(port, ids, c.nbits, bool(opt))
            assert ic.record(*table) == r["opt%d" % opt] and count == r["count"], (c, opt)


def test_generator_reproduces_fixture_where_the_reference_is_built():
    if not (oracle.have_reference("avx2") and oracle.have_reference("avx2_64")):
        return                                               # (the committed fixture is what the other tests check)
    r = subprocess.run([sys.executable, os.path.join(GOLDEN, "make_ids_golden.py"), "--check"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr


def _concat(tables):
    kinds = np.concatenate([t[1] for t in tables]); bits = np.concatenate([t[3] for t in tables]); gaps = np.concatenate([t[4] for t in tables])
    offs, nb, ng = [], 0, 0
    for _, k, o, b, g in tables:
        offs.append(np.where(k == ic.BIT, o + nb, np.where(k == ic.GAP, o + ng, 0)).astype(np.uint32))
        nb += b.size // ic.BW; ng += g.size
    return sum(t[0] for t in tables), kinds, np.concatenate(offs), bits, gaps


def test_window_tables_of_a_partition_concatenate_to_the_single_table():
    for c in ic.grid("I5") + [ic.CASES["I2/lds_16385"], ic.CASES["I4/u/touched_513"]]:
        nblocks = (c.size() + B - 1) // B
        parts = ic.I5_PARTITIONS if c.grid == "I5" else ((0, 16384, 16385), (0, 1, 16385)) if c.grid == "I2" else ((0, 100, 101, nblocks),)
        for opt in (False, True):
            whole = c.expected(opt)
            for cuts in parts:
                got = _concat([c.expected(opt, (f, t)) for f, t in zip(cuts[:-1], cuts[1:])])
                assert got[0] == whole[0] and all((a == b).all() and a.dtype == b.dtype for a, b in zip(got[1:], whole[1:])), (c, opt, cuts)
    c = ic.CASES["I5/s/mixed9"]
    assert len(ic.i5_windows()) == 55 + 6
    for f, t in ic.i5_windows():
        e = c.expected(True, (f, t))
        assert e[1].size == min(t, 9) - f and e[0] == max(min(c.nbits, min(t, 9) * B) - f * B, 0)
    for w in ((2, 3), (6, 7)):                                                         # windows that hold no id
        e = c.expected(True, w)
        assert e[0] == B and (e[1] == 0).all() and e[3].size == e[4].size == 0
    assert c.expected(True, (4, 4))[1].size == 0 and c.expected(True, (9, 12))[0] == 0
    with pytest.raises(ValueError):
        ic.expected_table(c.spec, c.nbits, True, (10, 12))
    # the size comes from the whole list, also where the largest id lies outside the window
    d = ic.CASES["I5/u/mixed9_sized_by_ids"]
    assert d.nbits == 0 and d.expected(True, (0, 2))[0] == 2 * B and d.expected(True, (8, ic.ALL))[0] == 65001
