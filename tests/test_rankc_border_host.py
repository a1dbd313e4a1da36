"""CPU: the constructed cases of rank compression (tests/golden/rankc_border_cases.py) are what they claim to be.  The three
thresholds the module uses are read from bmx_kernels15.h and bmx.hip; the NumPy transcription of the word network agrees with
bit-by-bit extract and deposit; plan() says of every border of the grids W, D, E and R that a named case meets it exactly; the
closed form of every case equals the oracle port (oracle_compress / oracle_decompress; the case past 2^32 through its one-block
twin), and the recorded reference subset (tests/golden/rankc_border_ref.json); where the reference is built the generator
reproduces the file.  The GPU module (tests/test_gpu_rankc_border.py) compares the kernels with the same cases."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import rankc_border_cases as rb
from rankc_border_cases import B, BIT, FULL, GAP, NULL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
FIXTURE = os.path.join(GOLDEN, "rankc_border_ref.json")
CASES = rb.cases()
PLANS = {}


def _plan(name):
    if name not in PLANS: PLANS[name] = rb.plan(CASES[name])
    return PLANS[name]


def test_constants_are_read_from_the_sources():
    k15 = open(os.path.join(rb.CSRC, "bmx_kernels15.h")).read()
    hip = open(os.path.join(rb.CSRC, "bmx.hip")).read()
    c = rb.read_constants()
    assert c == rb.CONSTANTS and (rb.NET_ROW, rb.EXT_NET_CA, rb.AUTO_PER_BLOCK) == tuple(c.values())
    assert re.search(r"^#define RANKC_NET_ROW %du\b" % rb.NET_ROW, k15, re.M)
    assert "const bool net = ca >= %du;" % rb.EXT_NET_CA in k15
    assert "total < (uint64_t)inb * %dull" % rb.AUTO_PER_BLOCK in hip
    assert 32 < rb.EXT_NET_CA <= rb.NET_ROW < 8192
    print("constants:", c)


def test_counts_hold():
    assert {g: len([c for c in CASES.values() if c.grid == g]) for g in rb.N_CASES} == rb.N_CASES
    assert rb.CATALOGUE.size == 263 and np.unique(rb.CATALOGUE).size == 249   # (the families overlap: 1 is a single bit and a prefix)
    for c in CASES.values():
        assert c.port_checked() or (c.grid == "R" and CASES[c.twin].port_checked()), c
        assert c.idx.table()[0].size == c.idx.nblocks


def test_word_network_transcription_agrees_with_bit_by_bit():
    """word_moves / word_extract_net / word_deposit_net as the header writes them, against the per-bit rule: every catalogue word
    under every catalogue word one bit at a time in Python, then 10^6 random pairs against the per-position loops"""
    cat = rb.CATALOGUE
    m, x = np.repeat(cat, cat.size), np.tile(cat, cat.size)
    en, dn = rb.word_extract_net(x, m), rb.word_deposit_net(x, m)
    el, dl = rb.word_extract_loop(x, m), rb.word_deposit_loop(x, m)
    assert (en == el).all() and (dn == dl).all()
    step = 37                                                   # one pair in 37 bit by bit in Python, every mask with several x
    for i in range(0, m.size, step):
        assert int(en[i]) == rb.bit_by_bit_extract(int(x[i]), int(m[i])) and int(dn[i]) == rb.bit_by_bit_deposit(int(x[i]), int(m[i])), i
    rng = np.random.default_rng(1)
    m = rng.integers(0, 1 << 32, 10 ** 6, dtype=np.uint64).astype(np.uint32)
    x = rng.integers(0, 1 << 32, 10 ** 6, dtype=np.uint64).astype(np.uint32)
    assert (rb.word_extract_net(x, m) == rb.word_extract_loop(x, m)).all()
    assert (rb.word_deposit_net(x, m) == rb.word_deposit_loop(x, m)).all()


def _block_words(v, b):
    bits = np.zeros(B, np.uint8); bits[v.offsets()[b]] = 1
    return np.packbits(bits, bitorder="little").view(np.uint32)


def test_grid_w_puts_every_word_through_both_forms():
    c = CASES["W/deposit"]; p = _plan(c.name)
    iw = _block_words(c.idx, 0).reshape(8, 256)
    for sname, _ in c.srcs:
        d = p["deposit"][sname][0]
        assert d["tot"] == [rb.NET_ROW - 1, rb.NET_ROW] * 4 and d["form"] == ["loop", "net"] * 4 and d["idx_kind"] == BIT, (c, sname, d)
        assert d["shortcut"] is None and d["start"] == 0
    seen = set()
    for q in range(4):
        part = {int(w) for w in rb.cat_part(q, 4)} - {0}
        assert 962 <= sum(bin(w).count("1") for w in part) <= 1135
        for row in (2 * q, 2 * q + 1):
            assert part <= {int(w) for w in iw[row]}, (q, row)
        seen |= part
    assert seen == {int(w) for w in rb.CATALOGUE} - {0}
    assert {s for s, _ in c.srcs} == {"random_half", "alternating", "ones_but_one"} and c.src("ones_but_one").ones.size == c.idx.count - 1

    c = CASES["W/extract"]; p = _plan(c.name)
    assert c.idx.count < B and [s for s, _ in c.srcs] == list(rb.EXT_VARIANTS)
    iw = np.concatenate([_block_words(c.idx, 0), _block_words(c.idx, 1)]).reshape(16, 256)
    for v in rb.EXT_VARIANTS:
        e = p["extract"][v][0]
        assert (e["b0"], e["b1"]) == (0, 1)
        for b in (0, 1):
            assert e["blocks"][b]["ca"] == [rb.EXT_NET_CA - 1, rb.EXT_NET_CA] * 4 and e["blocks"][b]["form"] == ["loop", "net"] * 4, (v, b)
        sw = np.concatenate([_block_words(c.src(v), 0), _block_words(c.src(v), 1)]).reshape(16, 256)
        assert ((sw & ~iw) == 0).all()
        for ei in range(8):
            part = rb.cat_part(ei, 8)
            sel = rb.select_bits(part, v, 100 + ei)
            for row in (2 * ei, 2 * ei + 1):
                got = {(int(m), int(s)) for m, s in zip(iw[row], sw[row]) if m != 0xFFFFFFFF and m}
                assert got == {(int(m), int(s)) for m, s in zip(part, sel) if m != 0xFFFFFFFF and m}, (v, row)
    low = rb.select_bits(rb.CATALOGUE, "lowest", 0); high = rb.select_bits(rb.CATALOGUE, "highest", 0)
    nz = rb.CATALOGUE != 0
    assert (rb.popcount32(low)[nz] == 1).all() and (rb.popcount32(high)[nz] == 1).all() and (low <= high).all()


def test_grid_d_meets_every_window_border():
    starts, lens, kinds = set(), set(), set()
    last_bit_65535 = last_bit_next0 = full_at_65535 = full_aligned = False
    for name in ("D/chain_small", "D/chain_big"):
        c = CASES[name]; p = _plan(name)
        assert len(p["deposit"]) == 3
        for sname, dep in p["deposit"].items():
            for b, s, ln in c.claims["windows"]:
                d = dep[b]
                assert (d["start"], d["len"]) == (s, ln), (c, sname, b, d)
                starts.add(s); lens.add(ln); kinds.add(d["idx_kind"])
                end = d["start"] + d["len"] - 1
                last_bit_65535 |= end == B - 1 and d["sb1"] == d["sb0"]
                last_bit_next0 |= end == B and d["sb1"] == d["sb0"] + 1
                if d["idx_kind"] == FULL and s == B - 1:
                    assert d["last_lds_word"] == 4095 and d["unaligned"]
                    full_at_65535 = True
                if d["idx_kind"] == FULL and s == 0:
                    assert not d["unaligned"] and d["sb1"] == d["sb0"]
                    full_aligned = True
                if s % 32: assert d["unaligned"]
    assert starts == set(rb.D_STARTS) == {0, 1, 31, 32, 33, 65504, 65535} and lens == {1, 2, 32, 33, 65535, 65536}
    assert {(s, ln) for n in ("D/chain_small", "D/chain_big") for _, s, ln in CASES[n].claims["windows"]} == \
        {(s, ln) for s in rb.D_STARTS for ln in lens}
    assert last_bit_65535 and last_bit_next0 and full_at_65535 and full_aligned
    assert kinds == {GAP, BIT, FULL}

    c = CASES["D/aligned_full"]
    for dep in _plan(c.name)["deposit"].values():
        assert sorted(dep) == [0, 1]
        for b, s, ln in c.claims["windows"]:
            d = dep[b]
            assert (d["start"], d["len"], d["idx_kind"], d["unaligned"], d["sb0"], d["sb1"]) == (s, ln, FULL, False, b, b) and d["shortcut"] is None

    c = CASES["D/kinds"]; p = _plan(c.name)
    dep = p["deposit"]["kinds"]
    pairs = set()
    for b in c.claims["straddling"]:
        d = dep[b]
        assert d["sb1"] == d["sb0"] + 1 and d["start"] == rb.D_KINDS_START and d["len"] == rb.D_KINDS_LEN, (b, d)
        pairs.add((d["d0"], d["d1"]))
        want = "null" if (d["d0"], d["d1"]) == (NULL, NULL) else "full" if (d["d0"], d["d1"]) == (FULL, FULL) else None
        assert d["shortcut"] == want, (b, d)
    assert pairs == {(a, b) for a in range(4) for b in range(4)}
    assert {dep[b]["idx_kind"] for b in c.claims["straddling"]} == {GAP, BIT}
    assert any(d["shortcut"] == "full" and d["sb1"] == d["sb0"] for d in dep.values())          # FULL with sb1 == sb0
    assert any(d["shortcut"] == "null" and d["sb1"] == d["sb0"] for d in dep.values())
    wa, wb = c.claims["near_miss"]
    for sname, all_of_it in (("ones_on_the_window", True), ("zero_on_the_window", False)):
        d = p["deposit"][sname]
        assert d[wa]["shortcut"] is None and (d[wa]["d0"], d[wa]["d1"]) == (BIT, BIT) and d[wa]["sb1"] != d[wa]["sb0"]
        assert d[wb]["shortcut"] is None and d[wb]["d0"] == BIT and d[wb]["sb1"] == d[wb]["sb0"]
        pos = rb.expected(c, sname, "decompress")["pos"]
        for w in (wa, wb):
            got = pos[(pos >> np.uint64(16)) == np.uint64(w)]
            want = np.uint64(w * B) + c.idx.offsets()[w].astype(np.uint64)
            assert (got.size == want.size and (got == want).all()) if all_of_it else got.size == 0, (sname, w)
    a = p["deposit"]["ends_at_sb1"][c.claims["source_end"]]
    assert a["d0_in_range"] and not a["d1_in_range"] and a["d0"] != NULL and a["d1"] == NULL and a["shortcut"] is None
    assert c.src("ends_at_sb1").nblocks == a["sb1"]
    z = p["deposit"]["ends_at_sb0"][c.claims["source_end"]]
    assert not z["d0_in_range"] and z["shortcut"] == "null" and c.src("ends_at_sb0").nblocks == z["sb0"]
    s = c.src("bits_around_count")
    cnt = c.idx.count
    assert {cnt - 1, cnt, cnt + 1} <= set(s.ones[-5:].tolist()) and s.nbits > cnt + B and int(s.ones[-1]) > cnt + B
    assert int(rb.expected(c, "bits_around_count", "decompress")["pos"][-1]) == int(c.idx.ones[-1])


def test_grid_e_meets_every_border_of_the_geometry():
    c = CASES["E/feeders"]; p = _plan(c.name)
    for sname in ("twin", "half", "firsts"):
        ext = p["extract"][sname]
        assert tuple(ext[t]["feeders"] for t in sorted(ext)) == rb.E_FEEDERS == (1, 2, 3, 4, 5, 8, 9)

    c = CASES["E/split"]; p = _plan(c.name)
    assert [(w, k) for _, w, k in c.claims["split_at"]] == [(40, 1), (300, 16), (1000, 31), (7, 0), (4, 0), (256, 0)]
    for sname in ("twin", "split_words_only"):
        ext = p["extract"][sname]
        for j, (b, w0, k) in enumerate(c.claims["split_at"], 1):
            if k:
                assert (b, w0, k) in ext[j]["lo_split"] and (b, w0, k) in ext[j - 1]["hi_split"], (sname, j, ext[j])
                assert ext[j]["b0"] == b == ext[j - 1]["b1"]
            else:
                assert (b, w0) in ext[j]["lo_word_border"] and not ext[j]["lo_split"] and not ext[j - 1]["hi_split"], (sname, j, ext[j])
                assert ext[j]["b0"] == b == ext[j - 1]["b1"] and ext[j]["first_offset"] == -16 * w0
        assert c.idx.block_kinds()[[b for b, _, _ in c.claims["split_at"]]].tolist() == [BIT] * 6

    c = CASES["E/ties"]; p = _plan(c.name)
    ext = p["extract"]["twin_without_block_11"]
    P = p["P"]
    assert [int(P[b]) for b in (1, 3, 4, 5, 8, 10, 12, 13, 15)] == [B, 2 * B, 2 * B, 3 * B, 3 * B, 4 * B, 5 * B, 6 * B - 1, 6 * B - 1]
    assert [ext[t]["ties_lo"] for t in range(1, 7)] == [1, 2, 4, 1, 1, 0]                    # followed by 0, 1 and 3 NULL blocks
    assert ext[5]["ties_hi"] == 3 and (ext[5]["b0"], ext[5]["b1"]) == (13, 16) and ext[6]["first_offset"] == -1 and ext[6]["b0"] == 16
    assert [(ext[t]["b0"], ext[t]["b1"]) for t in range(5)] == [(0, 1), (2, 3), (5, 5), (9, 10), (11, 12)]
    assert ext[4]["null_source_feeders"] == [c.claims["null_source_block"]] and ext[4]["ties_lo"] == 1
    assert c.src("short").nblocks == 3 < c.idx.nblocks and CASES["E/full_source"].src("full_short").nblocks == 1
    assert p["extract"]["short"][1]["null_source_feeders"] == [3]

    assert {_plan("E/total_%d" % t)["total"] for t in rb.E_TOTALS} == {1, 65535, 65536, 65537, 131072}
    for t in rb.E_TOTALS: assert CASES["E/total_%d" % t].claims["total"] == _plan("E/total_%d" % t)["total"] == t
    e1 = _plan("E/total_1")["extract"]["twin"][0]
    assert (e1["b0"], e1["b1"], e1["hi"]) == (1, 1, 1)

    c = CASES["E/shared_word"]; p = _plan(c.name)
    e = p["extract"]["twin"][0]
    assert e["feeders"] == 8 and p["total"] == 24 and sorted(e["blocks"]) == list(range(8))
    assert [e["blocks"][b]["offset"] for b in range(8)] == [3 * b for b in range(8)]              # all in image word 0, two per wave

    c = CASES["E/full_source"]; p = _plan(c.name)
    e = p["extract"]["full"][0]
    assert {(v["src_kind"], v["idx_kind"]) for v in e["blocks"].values()} == {(FULL, GAP), (FULL, BIT)} and e["null_source_feeders"] == [2]

    lo, at = _plan("E/auto_below"), _plan("E/auto_at")
    assert lo["total"] == lo["inb"] * rb.AUTO_PER_BLOCK - 1 and at["total"] == at["inb"] * rb.AUTO_PER_BLOCK and lo["inb"] == at["inb"] == 4
    assert (lo["auto_path"], at["auto_path"]) == (0, 1)


def test_grid_r_reaches_past_2_32_and_has_a_twin():
    big, twin = CASES["R/past_2_32"], CASES["R/twin"]
    H = 1 << 32
    assert big.idx.prefix == 65536 and twin.idx.prefix == 1 and big.twin == "R/twin" and big.flavour == "avx2_64"
    k = big.idx.block_kinds()
    assert k.size == 65540 and (k[:65536] == FULL).all() and k[65536:].tolist() == [BIT, GAP, FULL, BIT] and big.idx.count > H + B
    assert big.idx.table()[2].size == 2 * 2048                                                  # no slab for the prefix
    p = _plan(big.name)
    assert p["deposit"]["sparse_rank_space"][65536]["r0"] == H and p["deposit"]["sparse_rank_space"][65536]["sb0"] == 65536
    assert p["deposit"]["full_block_before_the_tail"][65535]["shortcut"] == "full"
    assert p["extract"]["sparse_index_space"][65536]["lo"] == H and p["extract"]["sparse_index_space"][65536]["b0"] == 65536
    pos = rb.expected(big, "sparse_index_space", "compress")["pos"]
    assert {H - 1, H, H + 1} <= set(pos.tolist()) and int(pos.max()) > H + 60000
    assert big.src("full_block_before_the_tail").block_kinds()[65535] == FULL
    for sname in ("sparse_rank_space", "blocks_around_the_prefix_end"):
        s = big.src(sname)
        assert {H - 1, H} <= set(s.ones.tolist())
        assert {65535, 65536} <= set((s.ones >> np.uint64(16)).tolist())
    for (sname, sb), (tname, st) in zip(big.srcs, twin.srcs):
        assert sname == tname
        for d in rb.DIRECTIONS:                        # beyond the prefix the twin's answer is the case's, moved by the prefix
            pb, pt = rb.expected(big, sname, d)["pos"], rb.expected(twin, sname, d)["pos"]
            tb, tt = pb[pb >= np.uint64(H - B)] - np.uint64(H - B), pt
            if sname == "sparse_index_space" or sname == "sparse_rank_space":
                tb, tt = pb[pb >= np.uint64(H - 2)] - np.uint64(H - B), pt[pt >= np.uint64(B - 2)]   # (the random prefix ids differ)
            assert tb.size == tt.size and (tb == tt).all() and tb.size > 2, (sname, d)


PORT_CASES = sorted(n for n, c in CASES.items() if c.port_checked())                           # all but R/past_2_32: its twin is an item


def test_every_case_is_port_checked_or_has_a_twin_that_is():
    assert [n for n in CASES if n not in PORT_CASES] == ["R/past_2_32"] and CASES["R/past_2_32"].twin in PORT_CASES


@pytest.mark.parametrize("name", PORT_CASES)
def test_closed_form_equals_the_oracle_port(port, name):
    c = CASES[name]
    for sname, _ in c.srcs:
        for d in rb.DIRECTIONS:
            assert rb.oracle_record(port, c, sname, d) == rb.expected_record(c, sname, d), (c, sname, d)


def test_recorded_reference_subset_equals_the_model():
    assert os.path.getsize(FIXTURE) < 100_000
    with open(FIXTURE) as f:
        fx = json.load(f)["cases"]
    rec = rb.recorded()
    assert sorted(fx) == sorted({c.name for c, _ in rec})
    names = {c.name for c, _ in rec}
    assert {"W/deposit", "W/extract", "D/kinds", "E/split", "E/ties"} <= names and len([n for n in names if n.startswith("R/")]) == 1
    assert fx["R/past_2_32"]["flavour"] == "avx2_64" and fx["R/past_2_32"]["idx_count"] > 1 << 32
    for c, sname in rec:
        r = fx[c.name]
        assert r["idx_count"] == c.idx.count and r["idx_nbits"] == c.idx.nbits and r["flavour"] == c.flavour
        for d in rb.DIRECTIONS:
            assert r["sources"][sname][d] == rb.expected_record(c, sname, d), (c, sname, d)
    assert sum(len(r["sources"]) for r in fx.values()) == len(rec)


def test_generator_reproduces_fixture_where_the_reference_is_built():
    import oracle
    if not (oracle.have_reference("avx2") and oracle.have_reference("avx2_64")):
        return                                               # (the committed fixture is what the other tests check)
    r = subprocess.run([sys.executable, os.path.join(GOLDEN, "make_rankc_border_golden.py"), "--check"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
