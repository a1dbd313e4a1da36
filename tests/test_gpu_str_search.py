"""GPU: string search over the resident planes of a bm::str_sparse_vector<> (bmx_slice_eq_keys and bitmagic_amd.str_scanner:
find_eq_str and its batch forms, src/bmsparsevec_algo.h:1194-1235, 2546-2588, 3263-3436).  Every case of str_cases.py is checked
three ways: against str_ref.json, against the NumPy model, and against the pipeline formulation on the device (one AND-SUB group per
string: an independent path).  The pipeline side takes the first PIPE_KEYS C-string keys of a case (a group per key: the 70,000
keys of the dictionary would be 70,000 groups of ~100 operands)."""
import ctypes as C
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import bitmagic_amd as bm  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import str_cases as sc_  # noqa: E402

B = 65536
U = np.uint64
BADARG, RANGE = 2, 3
PIPE_KEYS = 400
with open(os.path.join(ROOT, "tests", "golden", "str_ref.json")) as _f:
    FX = json.load(_f)["cases"]


@functools.lru_cache(maxsize=None)
def _model(name):
    return sc_.model_case(sc_.cases()[name])


def _check_entry(sc, case, name):
    """the batch entry against the fixture and the model: counts, first + found, and each output alone"""
    m, exp = _model(name), FX[name]
    counts, first, found = sc.eq_keys(case["keys"])
    assert sc_.sha(counts.astype("<u8")) == exp["counts_sha"] and int(counts.sum()) == exp["hits"], name
    assert sc_.sha(first.astype("<u8")) == exp["first_sha"] and int(found.sum()) == exp["n_found"], name
    assert np.array_equal(counts, m["counts"]) and np.array_equal(first, m["first"]) and np.array_equal(found.astype(bool), m["found"]), name
    only_c = sc.eq_keys(case["keys"], True, False)
    assert only_c[1] is None and only_c[2] is None and np.array_equal(only_c[0], counts)
    only_f = sc.eq_keys(case["keys"], False, True)
    assert only_f[0] is None and np.array_equal(only_f[1], first) and np.array_equal(only_f[2], found)
    return counts, first, found


def _check_pipeline(sc, case, name, counts, first, found):
    """the same keys as AND-SUB groups on the device: a counts pipeline, find_first_and_sub and an index-list pipeline"""
    m = _model(name)
    strs = sc_.key_strings(case)
    qs = [q for q in range(len(strs)) if q not in case["entry_only"]][:PIPE_KEYS]
    if not qs:
        return
    sel = [strs[q] for q in qs]
    pc = sc.find_eq_str_counts(sel, use_pipeline=True)
    assert np.array_equal(pc, counts[qs]), name
    few = qs[:24]
    pos, fnd = sc.find_eq_str_first([strs[q] for q in few], use_pipeline=True)
    assert np.array_equal(pos, first[few]) and np.array_equal(fnd, found[few].astype(bool)), name
    off, ids = sc.find_eq_str_indices(sel)
    assert np.array_equal(np.diff(off.astype(np.int64)), counts[qs].astype(np.int64)), name
    for k, q in enumerate(qs):
        assert np.array_equal(ids[int(off[k]):int(off[k + 1])], m["ids"][int(m["offsets"][q]):int(m["offsets"][q + 1])]), (name, q)
    if len(qs) == len(strs):                                             # every key went through: the whole CSR is the fixture's
        assert sc_.sha(off.astype("<u8")) == FX[name]["offsets_sha"] and sc_.sha(ids.astype("<u8")) == FX[name]["ids_sha"], name


@pytest.mark.parametrize("name", sorted(FX))
def test_fixture_case(ctx, name):
    case = sc_.cases()[name]
    assert FX[name] == dict(sc_.record(case, _model(name), bm.str_search_groups), anchored=FX[name]["anchored"])      # the fixture is the model's
    sc, _ = sc_.device_scanner(bm, ctx, case)
    got = _check_entry(sc, case, name)
    if case["keys"].shape[0]:
        _check_pipeline(sc, case, name, *got)


def test_grid_holds_every_block_kind(ctx):
    case = sc_.cases()["grid"]
    _, vecs = sc_.device_scanner(bm, ctx, case)
    kinds = np.zeros(4, np.int64)
    for k, v in vecs.items():
        if k != "nn":
            kinds += np.array(v.info()["counts"], np.int64)
    assert (kinds > 0).all(), kinds                                      # NULL, FULL, bit and GAP blocks among the planes
    assert vecs["p22"].info()["nblocks"] == 13 and case["planes"][13] is None


def test_single_searches_and_first(ctx):
    """find_eq_str / find_eq_str_prefix / find_first_eq_str over the `first` and the pool column"""
    case = sc_.cases()["first"]
    sc, _ = sc_.device_scanner(bm, ctx, case)
    m = _model("first")
    for q, s in enumerate(sc_.key_strings(case)):
        bv, f = sc.find_eq_str(s)
        rows = bv.to_indices() if (f and bv is not None) else np.zeros(0, U)
        assert np.array_equal(rows, m["ids"][int(m["offsets"][q]):int(m["offsets"][q + 1])]), s
        assert sc.find_first_eq_str(s) == (bool(m["found"][q]), int(m["first"][q])), s
    octets = sc_.row_octets(case, 8)
    for prefix in (b"first", b"firs", b"l", b"never", b""):
        bv, f = sc.find_eq_str_prefix(prefix)
        exp = np.flatnonzero((octets[:, :len(prefix)] == np.frombuffer(prefix, np.uint8)).all(axis=1)).astype(U)
        got = bv.to_indices() if (f and bv is not None) else np.zeros(0, U)
        assert np.array_equal(got, exp), prefix
    assert sc.find_eq_str_prefix(b"firs")[0].count() >= 4 > sc.find_eq_str(b"firs")[0].count()
    # the empty string: with and without the not-NULL vector
    for name in ("keys_empty_with_nn", "keys_empty_without_nn"):
        c2 = sc_.cases()[name]
        s2, _ = sc_.device_scanner(bm, ctx, c2)
        m2 = _model(name)
        bv, f = s2.find_eq_str(b"")
        assert f and bv.count() == m2["counts"][0] and s2.find_first_eq_str(b"") == (True, int(m2["first"][0]))


def test_facade_chooses_the_batch_entry(ctx):
    """without use_pipeline the batch functions take bmx_slice_eq_keys from BATCH_MIN strings upward; both routes agree"""
    from bitmagic_amd import _str_scanner
    case = sc_.cases()["keys_n300"]
    sc, _ = sc_.device_scanner(bm, ctx, case)
    m = _model("keys_n300")
    strs = sc_.key_strings(case)
    calls = []
    orig = sc.eq_keys
    sc.eq_keys = lambda *a, **k: (calls.append(1), orig(*a, **k))[1]
    big, small = strs, strs[:_str_scanner.BATCH_MIN - 1]
    assert np.array_equal(sc.find_eq_str_counts(big), m["counts"]) and len(calls) == 1
    pos, fnd = sc.find_eq_str_first(big)
    assert np.array_equal(pos, m["first"]) and np.array_equal(fnd, m["found"]) and len(calls) == 2
    assert np.array_equal(sc.find_eq_str_counts(small), m["counts"][:len(small)]) and len(calls) == 2      # a short batch: the pipeline
    assert np.array_equal(sc.find_eq_str_counts(big, use_pipeline=True), m["counts"]) and len(calls) == 2
    assert sc.find_eq_str_counts([]).size == 0 and len(calls) == 2


def test_remap_table(ctx):
    """a column of CODES (remap_matrix2_: one 256-entry table per octet position); a character the position never holds, and a
    string longer than the table, are found nowhere"""
    rng = np.random.default_rng(5)
    words = [b"ga", b"tag", b"gat", b"a", b"tt"]
    size = B + 300
    pick = rng.integers(0, len(words), size)
    table = np.zeros((3, 256), np.uint8)
    for j in range(3):
        for code, ch in enumerate(sorted({w[j] for w in words if len(w) > j}), 1):
            table[j, ch] = code
    coded = sc_.pad([bytes(int(table[j, ch]) for j, ch in enumerate(w)) for w in words], 3)[pick]
    vecs = {k: bm.bit_import_u32(ctx, sc_.words_of(ids, n), True) for k, (ids, n) in sc_._planes_of(coded, 18).items()}
    planes = [vecs["p%d" % p] if (p & 7) < 2 else None for p in range(18)]                        # codes 1..3: two planes per octet
    sc = bm.str_scanner(ctx, planes, size=size).set_remap(table.tobytes(), 3)
    queries = words + [b"gaa", b"tagg", b"x", b"g", b"ta"] * 12
    exp = np.array([int((pick == words.index(w)).sum()) if w in words else 0 for w in queries], U)
    from bitmagic_amd import _str_scanner
    assert len(queries) >= _str_scanner.BATCH_MIN                       # the default route is the batch entry
    assert np.array_equal(sc.find_eq_str_counts(queries), exp) and np.array_equal(sc.find_eq_str_counts(queries, use_pipeline=True), exp)
    pos, fnd = sc.find_eq_str_first(queries)
    for q, w in enumerate(queries):
        assert bool(fnd[q]) == (w in words) and (not fnd[q] or pos[q] == np.flatnonzero(pick == words.index(w))[0]), w
        assert sc.find_first_eq_str(w) == (bool(fnd[q]), int(pos[q])), w
    bv, f = sc.find_eq_str_prefix(b"ga")
    assert f and bv.count() == exp[0] + exp[2]                            # "ga" and "gat"


def _rerun(ctx, names, key, value):
    """the cases again under a tuning key: identical answers"""
    try:
        ctx.set_tuning(key, value)
        for name in names:
            case = sc_.cases()[name]
            sc, _ = sc_.device_scanner(bm, ctx, case)
            _check_entry(sc, case, name)
    finally:
        ctx.set_tuning(key, {"eqk_expand_kb": 256 * 1024}.get(key, 0))


def test_hook_four_fingerprint_bits(ctx):
    """eqk_fp_bits = 4: sixteen fingerprints for all the keys, the exact verification decides nearly every row"""
    _rerun(ctx, ["grid", "dictionary"] + sorted(n for n in FX if n.startswith("keys_")), "eqk_fp_bits", 4)


def test_hook_keys_per_pass(ctx):
    _rerun(ctx, ["keys_n300", "keys_n65"], "eqk_pass_keys", 64)          # 5 passes; 2 passes of 33 and 32


def test_hook_expansion_windows(ctx):
    """the grid's GAP-holding planes expanded 4 block columns at a time: 4 windows; and one column at a time"""
    case = sc_.cases()["grid"]
    gap_planes = sum(1 for k, (ids, _) in case["vecs"].items() if k != "nn")
    _rerun(ctx, ["grid"], "eqk_expand_kb", gap_planes * 8 * 4)
    _rerun(ctx, ["grid", "tail_65537"], "eqk_expand_kb", 0)


def test_arguments(ctx):
    case = sc_.cases()["keys_n2"]
    sc, vecs = sc_.device_scanner(bm, ctx, case)
    L = bm.lib()
    p = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None
    arr = (C.c_void_p * len(sc.planes))(*[v._h if v is not None else None for v in sc.planes])
    keys = case["keys"]
    out = lambda: (np.full(2, 77, U), np.full(2, 77, U), np.full(2, 77, np.uint8))
    call = lambda a, n_planes, size, nn, k, kb, n, c, f, fd: L.bmx_slice_eq_keys(ctx._h, a, n_planes, size, nn, p(k), kb, n, p(c), p(f), p(fd))
    c, f, fd = out()
    assert call(arr, len(sc.planes), sc.size(), None, keys, 7, 0, c, f, fd) == 0 and c[0] == f[0] == fd[0] == 77      # n == 0: nothing written
    assert call(arr, len(sc.planes), sc.size(), None, None, 7, 0, None, None, None) == 0
    assert call(arr, len(sc.planes), sc.size(), None, None, 7, 2, c, f, fd) == BADARG
    assert call(arr, len(sc.planes), sc.size(), None, keys, 7, 2, None, None, None) == BADARG
    big = (C.c_void_p * 1025)()
    assert call(big, 1025, sc.size(), None, keys, 7, 2, c, f, fd) == RANGE
    assert call(big, 1024, sc.size(), None, keys, 7, 2, c, f, fd) == 0 and c.tolist() == [0, 0]      # 1,024 absent planes: nothing matches
    assert call(arr, len(sc.planes), (1 << 36) + 1, None, keys, 7, 2, c, f, fd) == RANGE
    other = bm.context(0)
    try:
        foreign = bm.bit_import_u32(other, np.zeros(2048, np.uint32), True)
        a2 = (C.c_void_p * len(sc.planes))(*[v._h if v is not None else None for v in sc.planes])
        a2[3] = foreign._h
        assert call(a2, len(sc.planes), sc.size(), None, keys, 7, 2, c, f, fd) == BADARG
        assert call(arr, len(sc.planes), sc.size(), foreign._h, keys, 7, 2, c, f, fd) == BADARG
        del foreign
    finally:
        other.close()
    # size == 0 and nslices == 0 are ordinary inputs
    c, f, fd = out()
    assert call(arr, len(sc.planes), 0, None, keys, 7, 2, c, f, fd) == 0 and c.tolist() == [0, 0] and fd.tolist() == [0, 0]
    z = np.zeros((2, 1), np.uint8); z[1, 0] = 5
    assert call(None, 0, 1000, None, z, 1, 2, c, f, fd) == 0 and c.tolist() == [1000, 0] and f.tolist() == [0, 0] and fd.tolist() == [1, 0]
    for key, bad in (("eqk_fp_bits", 33), ("eqk_fp_bits", -1), ("eqk_pass_keys", -1), ("eqk_expand_kb", -1)):
        with pytest.raises(bm.BmxError) as e:
            ctx.set_tuning(key, bad)
        assert e.value.status == BADARG


_REDZONE_SCRIPT = r'''
import json, os, sys
sys.path.insert(0, os.getcwd())
sys.path.insert(0, os.path.join(os.getcwd(), "tests", "golden"))
import numpy as np
import bitmagic_amd as bm
import str_cases as sc_
fx = json.load(open(os.path.join("tests", "golden", "str_ref.json")))["cases"]
ctx = bm.context(0)
out = {"enabled": ctx.redzone_check()["enabled"], "ok": True}
for name, kb in (("grid", 256 * 1024), ("grid", 1248), ("keys_n300", 256 * 1024)):
    ctx.set_tuning("eqk_expand_kb", kb)
    case = sc_.cases()[name]
    sc, vecs = sc_.device_scanner(bm, ctx, case)
    counts, first, found = sc.eq_keys(case["keys"])
    out["ok"] = out["ok"] and sc_.sha(counts.astype("<u8")) == fx[name]["counts_sha"] and sc_.sha(first.astype("<u8")) == fx[name]["first_sha"]
    del sc, vecs
ctx.synchronize()
out["hits"] = ctx.redzone_check()["hits"]
print("REDZONE " + json.dumps(out))
'''


def test_red_zones_clean():
    """a fresh process under BMX_DEBUG_REDZONE=1: the grid (one window and four) and a 300-key batch write nothing outside their
    allocations"""
    env = dict(os.environ, BMX_DEBUG_REDZONE="1")
    r = subprocess.run([sys.executable, "-c", _REDZONE_SCRIPT], capture_output=True, text=True, timeout=600, cwd=ROOT, env=env)
    line = [l for l in r.stdout.splitlines() if l.startswith("REDZONE ")]
    assert r.returncode == 0 and line, (r.stdout + r.stderr)[-3000:]
    out = json.loads(line[0][8:])
    assert out["enabled"] and out["hits"] == 0, out
    assert out["ok"], out
