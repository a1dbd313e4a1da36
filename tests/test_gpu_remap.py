"""GPU: the values of the selected rows of a resident bit-sliced column and the image of a row set under it (bmx_slice_values,
bmx_slice_values_dev, bmx_slice_remap and the Python facade over them: set2set_11_transform::remap, src/bmsparsevec_algo.h:2096-2205)
against remap_ref.json and the NumPy model of remap_cases.py.  Every fixture case runs; content is compared by the hashes of the
row ids, of the values in row order and of the ascending image.

A value of 40 bits lies beyond the 2^20 blocks a device vector can hold: the value LIST carries it at width 8
(test_wide_values_and_the_block_limit), its image is BMX_ERR_RANGE, and the image value in a high output block is the 36-bit one
of case wide_36."""
import ctypes as C
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
import remap_cases as rc_  # noqa: E402

B = 65536
U = np.uint64
BADALLOC, BADARG, RANGE = 1, 2, 3
with open(os.path.join(ROOT, "tests", "golden", "remap_ref.json")) as _f:
    FX = json.load(_f)["cases"]


def _raw_values(ctx, sc, sel, width, cap, want_rows=True, fill=0xA5):
    """one call of bmx_slice_values into buffers of cap entries pre-filled with a pattern -> (status, n, values, rows)"""
    dt = np.uint32 if width == 4 else np.uint64
    vals, rows = np.full(max(cap, 1), fill, dt), np.full(max(cap, 1), fill, dt)
    n = C.c_uint64(12345)
    st = bm.lib().bmx_slice_values(*sc._values_args(sel), width, bm._ptr(vals) if cap else None, bm._ptr(rows) if (cap and want_rows) else None,
                                   cap, C.byref(n))
    return st, n.value, vals, rows


def _raw_remap(ctx, sc, sel, nbits=0, optimize=1, want_n=True):
    h, n = C.c_void_p(), C.c_uint64(12345)
    st = bm.lib().bmx_slice_remap(*sc._values_args(sel), nbits, optimize, C.byref(h), C.byref(n) if want_n else None)
    return st, (bm.bvector(ctx, h) if h.value else None), n.value


def _check(ctx, case, exp):
    sc, sel, _ = rc_.device_scanner(bm, ctx, case)
    vals, rows = sc.values(sel, rows=True)
    assert vals.size == rows.size == exp["n_rows"]
    assert vals.dtype == (np.uint32 if len(case["planes"]) <= 32 else np.uint64)
    assert rc_.sha(rows.astype("<u8")) == exp["rows_sha"]
    assert rc_.sha(vals.astype("<u8")) == exp["values_sha"]
    only = sc.values(sel)
    assert np.array_equal(only, vals)
    if len(case["planes"]) <= 32:                                        # the same list at width 8
        st, n, v8, r8 = _raw_values(ctx, sc, sel, 8, exp["n_rows"])
        assert st == 0 and n == exp["n_rows"]
        assert rc_.sha(v8[:n].astype("<u8")) == exp["values_sha"] and rc_.sha(r8[:n].astype("<u8")) == exp["rows_sha"]
    st, img, n_rows = _raw_remap(ctx, sc, sel)
    if exp["image_max"] is not None and exp["image_max"] >= rc_.IMAGE_LIMIT:        # no device vector holds that position
        assert st == RANGE and img is None and n_rows == 0
        return sc, sel, None
    assert st == 0 and n_rows == exp["n_rows"]
    ids = img.to_indices()
    st, img, n_rows = _raw_remap(ctx, sc, sel)
    assert st == 0 and n_rows == exp["n_rows"]
    ids = img.to_indices()
    assert ids.size == exp["image_count"] == img.count() and rc_.sha(ids.astype("<u8")) == exp["image_sha"]
    assert img.size() == (exp["image_max"] + 1 if exp["image_max"] is not None else 0)
    return sc, sel, img


@pytest.mark.parametrize("name", sorted(FX))
def test_fixture_case(ctx, name):
    case = rc_.cases()[name]
    assert FX[name] == dict(rc_.record(rc_.model_case(case)), anchored=FX[name]["anchored"])      # the fixture is the model's
    _check(ctx, case, FX[name])


def test_every_case_has_a_record():
    assert sorted(FX) == sorted(rc_.cases())


def test_grid_operands_hold_the_planned_kinds(ctx):
    case = rc_.cases()["grid"]
    vecs = rc_.device_vecs(bm, ctx, case)
    plan = {0: bm.NULL, 1: bm.FULL, 2: bm.GAP, 3: bm.BIT}
    q = [k + 1 for k in range(15)]
    for key, f in (("sel", lambda x: x & 3), ("nn", lambda x: x >> 2), ("p0", lambda x: (x + 1) & 3), ("p1", lambda x: (x >> 1) & 3)):
        kinds = [int(k) for k in vecs[key].block_table()[0]]
        # (the last column is cut at size: a FULL plan becomes one run, a GAP block)
        assert kinds[:14] == [plan[f(x)] for x in q[:14]], key
    sweep = rc_.cases()["sweep"]
    sk = [int(k) for k in rc_.device_vecs(bm, ctx, {"vecs": {"sel": sweep["vecs"]["sel"]}, "bit_keys": frozenset()})["sel"].block_table()[0]]
    assert [k == bm.FULL for k in sk] == [n == B for n in rc_.SWEEP_COUNTS] and len(sk) == 33


def test_capacity_protocol(ctx):
    """cap = n - 1, n and 0 for both entries: *n is always the number needed; too small writes nothing"""
    import torch
    case = rc_.cases()["sel_longer"]
    sc, sel, _ = rc_.device_scanner(bm, ctx, case)
    m = rc_.model_case(case)
    n = m["rows"].size
    assert n > 2
    for width in (4, 8):
        dt = np.uint32 if width == 4 else np.uint64
        for cap in (n - 1, 0):
            st, got_n, vals, rows = _raw_values(ctx, sc, sel, width, cap)
            assert st == RANGE and got_n == n
            assert (vals == dt(0xA5)).all() and (rows == dt(0xA5)).all()
        st, got_n, vals, rows = _raw_values(ctx, sc, sel, width, n)
        assert st == 0 and got_n == n and np.array_equal(vals.astype(U), m["values"]) and np.array_equal(rows.astype(U), m["rows"])
        st, got_n, vals, rows = _raw_values(ctx, sc, sel, width, n + 3, want_rows=False)
        assert st == 0 and got_n == n and np.array_equal(vals[:n].astype(U), m["values"]) and (vals[n:] == dt(0xA5)).all() and (rows == dt(0xA5)).all()
        # the device entry
        tdt = torch.int32 if width == 4 else torch.int64
        d_val = torch.full((n + 4,), -1, dtype=tdt, device="cuda")
        d_row = torch.full((n + 4,), -1, dtype=tdt, device="cuda")
        torch.cuda.synchronize()
        for cap in (n - 1, 0):
            with pytest.raises(bm.BmxError) as e:
                sc.values_dev(d_val.data_ptr(), cap, sel, d_row.data_ptr(), width)
            ctx.synchronize()
            assert e.value.status == RANGE and bool((d_val == -1).all()) and bool((d_row == -1).all())
        assert sc.values_dev(d_val.data_ptr(), n, sel, d_row.data_ptr(), width) == n
        ctx.synchronize()
        gv, gr = d_val.cpu().numpy().view(dt), d_row.cpu().numpy().view(dt)
        assert np.array_equal(gv[:n].astype(U), m["values"]) and np.array_equal(gr[:n].astype(U), m["rows"])
        assert (d_val.cpu().numpy()[n:] == -1).all() and (d_row.cpu().numpy()[n:] == -1).all()
        d_val.fill_(-1); torch.cuda.synchronize()
        assert sc.values_dev(d_val.data_ptr(), n + 4, sel, None, width) == n                 # no row list
        ctx.synchronize()
        assert np.array_equal(d_val.cpu().numpy().view(dt)[:n].astype(U), m["values"])


def test_size_rule_and_n_rows(ctx):
    """nbits_out smaller and larger than the image; n_rows may be left out; an empty selection is all-NULL of nbits_out bits"""
    case = rc_.cases()["m_to_1"]
    sc, sel, _ = rc_.device_scanner(bm, ctx, case)
    m = rc_.model_case(case)
    top = int(m["image"].max())
    for nbits, size in ((0, top + 1), (top - 3, top + 1), (top + 1, top + 1), (5 * B + 7, 5 * B + 7)):
        st, img, n_rows = _raw_remap(ctx, sc, sel, nbits)
        assert st == 0 and n_rows == m["rows"].size and img.size() == size
        assert np.array_equal(img.to_indices(), m["image"])
    st, img, n_rows = _raw_remap(ctx, sc, sel, want_n=False)
    assert st == 0 and n_rows == 12345 and np.array_equal(img.to_indices(), m["image"])
    empty = bm.bvector.from_indices(ctx, np.zeros(0, np.uint32), case["size"])
    for nbits in (0, 3 * B + 1):
        st, img, n_rows = _raw_remap(ctx, sc, empty, nbits)
        assert st == 0 and n_rows == 0 and img.size() == nbits and img.count() == 0
        assert all(int(k) == bm.NULL for k in img.block_table()[0])


@pytest.mark.parametrize("name", ["m_to_1", "sweep", "grid", "max_u32", "wide_36"])
def test_optimize_gives_the_kinds_of_from_indices(ctx, name):
    """optimize = 0 / 1: block for block the kinds bmx_vec_from_indices gives for the same (unsorted, duplicated) list"""
    case = rc_.cases()[name]
    sc, sel, _ = rc_.device_scanner(bm, ctx, case)
    vals = sc.values(sel)
    for opt in (0, 1):
        st, img, _ = _raw_remap(ctx, sc, sel, 0, opt)
        assert st == 0
        ref = bm.bvector.from_indices(ctx, vals, 0, bm.BM_UNSORTED, bool(opt))
        assert img.size() == ref.size()
        assert np.array_equal(img.block_table()[0], ref.block_table()[0]), opt
        assert bm.count_xor(img, ref) == 0


def _random_case(seed: int):
    rng = np.random.default_rng(seed)
    size = int(rng.integers(1, 4 * B))
    nblk = (size + B - 1) // B
    nplanes = int(rng.integers(1, 6 if seed % 2 == 0 else 12))          # (even seeds: at most 32 image values, all of them probed)
    vecs, planes = {}, []
    for i in range(nplanes):
        if rng.random() < 0.15:
            planes.append(None); continue
        vecs["p%d" % i] = rc_._cut(rc_._mixed(seed * 100 + i, nblk), size)
        planes.append("p%d" % i)
    nn = sel = None
    if rng.random() < 0.6:
        nn = "nn"; vecs[nn] = rc_._cut(rc_._mixed(seed * 100 + 90, nblk), size)
    if rng.random() < 0.8:
        sel = "sel"; vecs[sel] = rc_._mixed(seed * 100 + 91, nblk + int(rng.integers(0, 2)))
    return rc_._case(vecs, planes, size, nn, sel)


@pytest.mark.parametrize("seed", range(10))
def test_random_columns_device_only_consistency(ctx, seed):
    """the model, then two statements that need no model: from_indices(values(mask)) == remap(mask), and every image value is
    found by find_eq among the selected rows, the counts adding up to n_rows"""
    case = _random_case(2000 + seed)
    m = rc_.model_case(case)
    sc, sel, img = _check(ctx, case, rc_.record(m))
    st, _, n_rows = _raw_remap(ctx, sc, sel)
    vals = sc.values(sel)
    again = bm.bvector.from_indices(ctx, vals, 0, bm.BM_UNSORTED, True)
    assert again.size() == img.size() and bm.count_xor(again, img) == 0
    mask = sel
    if mask is None:
        mask = bm.bvector.from_ranges(ctx, np.array([[0, case["size"] - 1]], U), case["size"])
    if sc.not_null is not None:                                          # (the random planes do not hold 0 in NULL rows: find_eq of a
        mask = bm.bvector.bit_and(mask, sc.not_null)                     # non-zero value would count them)
    total = 0
    for v in img.to_indices()[:64]:
        hit, found = sc.find_eq(int(v))
        c = bm.count_and(hit, mask) if (found and hit is not None) else 0
        assert c > 0, int(v)
        total += c
    if img.count() <= 64:                                                # (selector rows beyond size match nothing: find_eq ends at size)
        assert total == n_rows


def test_wide_values_and_the_block_limit(ctx):
    """a 40-bit value: the list carries it at width 8; no device vector holds position 2^39, so the image is BMX_ERR_RANGE and
    nothing stays allocated; the same for nbits_out beyond 2^36; width 4 cannot carry more than 32 planes"""
    rows = 2000
    v = np.arange(rows, dtype=U) * U(3)
    v[[17, 1500]] = (U(1) << U(39)) + U(5)
    case = rc_._from_values(v, np.zeros(rows, bool), np.arange(0, rows, 5), nplanes=40)
    sc, sel, _ = rc_.device_scanner(bm, ctx, case)
    m = rc_.model_case(case)
    assert int(m["image"].max()) == (1 << 39) + 5
    vals, ids = sc.values(sel, rows=True)
    assert vals.dtype == np.uint64 and np.array_equal(vals, m["values"]) and np.array_equal(ids, m["rows"])
    ctx.synchronize(); ctx.trim()
    base = ctx.mem_used()
    st, img, n_rows = _raw_remap(ctx, sc, sel)
    assert st == RANGE and img is None and n_rows == 0
    st, img, _ = _raw_remap(ctx, sc, sel, nbits=(1 << 36) + 1)
    assert st == RANGE and img is None
    ctx.synchronize(); ctx.trim()
    assert ctx.mem_used() == base
    st, n, _, _ = _raw_values(ctx, sc, sel, 4, rows)                      # 40 planes at width 4
    assert st == BADARG
    below = bm.bvector.from_indices(ctx, np.array([0, 5, 10], np.uint32), rows)      # the rows below the wide ones still map
    st, img, n_rows = _raw_remap(ctx, sc, below)
    assert st == 0 and n_rows == 3 and list(img.to_indices()) == [0, 15, 30]


def test_bad_arguments_and_no_leak(ctx):
    case = rc_.cases()["sel_longer"]
    sc, sel, vecs = rc_.device_scanner(bm, ctx, case)
    other = bm.context(0)
    foreign = bm.bit_import_u32(other, rc_.case_words(case, "p0"), True)
    L = bm.lib()
    args = sc._values_args(sel)
    n, h = C.c_uint64(), C.c_void_p()
    buf = np.zeros(8, U)
    assert _raw_remap(ctx, sc, sel)[0] == 0 and sc.values(sel).size
    ctx.synchronize(); ctx.trim()
    base = ctx.mem_used()

    def refused(st, code=BADARG):
        assert st == code and h.value is None
        ctx.synchronize(); ctx.trim()
        assert ctx.mem_used() == base

    many = (C.c_void_p * 65)()
    vals = lambda a, w=4: L.bmx_slice_values(*a, w, bm._ptr(buf), None, 1, C.byref(n))
    remap = lambda a: L.bmx_slice_remap(*a, 0, 1, C.byref(h), C.byref(n))
    for fn in (vals, remap):
        refused(fn([None] + args[1:]))                                                   # null context
        bad = list(args); arr = (C.c_void_p * 4)(); bad[1] = arr
        for i in range(4):
            arr[i] = foreign._h if i == 0 else args[1][i]
        refused(fn(bad))                                                                 # a plane of another context
        bad = list(args); bad[4] = foreign._h
        refused(fn(bad))                                                                 # ... as the not-NULL vector
        bad = list(args); bad[5] = foreign._h
        refused(fn(bad))                                                                 # ... as the selector
        bad = list(args); bad[1] = many; bad[2] = 65
        refused(fn(bad))                                                                 # more than 64 planes
    bad = list(args); bad[1] = many; bad[2] = 33
    refused(vals(bad, 4))                                                                # width 4 with 33 planes
    assert vals(bad, 8) == RANGE and n.value > 1                                         # ... fine at width 8 (cap 1 is too small)
    refused(vals(args, 2)); refused(vals(args, 16))                                      # width
    refused(L.bmx_slice_values(*args, 4, bm._ptr(buf), None, 1, None))                   # n
    refused(L.bmx_slice_values(*args, 4, None, None, 1, C.byref(n)))                     # no buffer with cap > 0
    refused(L.bmx_slice_remap(*args, 0, 1, None, C.byref(n)))                            # result
    # success: the image is the only thing that stays, and it goes with its handle
    img = bm.set2set_11_transform(ctx).remap(sel, sc)
    ctx.synchronize()
    assert ctx.mem_used() > base
    del img
    sc.values(sel, rows=True)
    ctx.synchronize(); ctx.trim()
    assert ctx.mem_used() == base
    del foreign
    other.close()


@pytest.mark.parametrize("kind", [4, 6])
def test_allocation_failures_leave_nothing(ctx, kind):
    """every device allocation of the three entries fails in turn (kind 4: it fails, 6: it throws std::bad_alloc):
    BMX_ERR_BADALLOC, no result, bmx_ctx_mem_used unchanged, and the next call works"""
    case = rc_.cases()["sel_longer"]
    sc, sel, _ = rc_.device_scanner(bm, ctx, case)
    m = rc_.model_case(case)
    n = m["rows"].size
    L = bm.lib()
    args = sc._values_args(sel)
    for which in ("values", "remap"):
        ctx.synchronize(); ctx.trim()
        base = ctx.mem_used()
        failed, k = 0, 0
        while True:
            h, cnt = C.c_void_p(), C.c_uint64()
            vals, rows = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
            ctx.inject_failure(kind, k)
            try:
                if which == "values":
                    st = L.bmx_slice_values(*args, 4, bm._ptr(vals), bm._ptr(rows), n, C.byref(cnt))
                else:
                    st = L.bmx_slice_remap(*args, 0, 1, C.byref(h), C.byref(cnt))
            finally:
                ctx.inject_failure(0, 0)
            ctx.synchronize()
            if st == 0:
                break
            assert st == BADALLOC and h.value is None, (which, k, st)
            ctx.trim()
            assert ctx.mem_used() == base, (which, k, ctx.mem_used() - base)
            failed += 1; k += 1
            assert k < 100
        assert failed >= (5 if which == "values" else 6), (which, failed)   # table, counts, starts, the lists; + the vector's
        if which == "values":
            assert cnt.value == n and np.array_equal(vals.astype(U), m["values"]) and np.array_equal(rows.astype(U), m["rows"])
        else:
            img = bm.bvector(ctx, h)
            assert cnt.value == n and np.array_equal(img.to_indices(), m["image"])
            del img
        ctx.synchronize(); ctx.trim()
        assert ctx.mem_used() == base


def test_python_facade(ctx):
    case = rc_.cases()["zero_with_nn"]
    sc, sel, vecs = rc_.device_scanner(bm, ctx, case)
    m = rc_.model_case(case)
    t = bm.set2set_11_transform(ctx)
    img = t.remap(sel, sc)
    assert isinstance(img, bm.bvector) and np.array_equal(img.to_indices(), m["image"]) and t.n_rows == m["rows"].size
    assert np.array_equal(t.run(sel, sc, nbits=B).to_indices(), m["image"])
    with pytest.raises(bm.BmxError) as e:
        t.remap(sel)
    assert e.value.status == BADARG
    t.attach_sv(sc, compute_stats=True)
    assert np.array_equal(t.remap(sel).to_indices(), m["image"])
    every = t.remap(None)                                                 # every row
    assert np.array_equal(every.to_indices(), np.unique(case["values"][0][~case["values"][1]]))
    t.attach_sv(None)
    with pytest.raises(bm.BmxError):
        t.remap(sel)
    # value 0 without a not-NULL vector: bit 0 of the image (src/bmsparsevec_algo.h:2142-2163); with one, NULL rows drop out
    c0 = rc_.cases()["only_zero_without_nn"]
    s0, sel0, _ = rc_.device_scanner(bm, ctx, c0)
    assert list(t.remap(sel0, s0).to_indices()) == [0]
    c1 = rc_.cases()["only_zero_with_nn_all_null"]
    s1, sel1, _ = rc_.device_scanner(bm, ctx, c1)
    assert t.remap(sel1, s1).count() == 0 and t.n_rows == 0
    # a signed column: values() converts the s2u patterns, remap is refused
    sv = np.array([0, -1, 5, -7, 100, -(1 << 20), 3], np.int64)
    pat = np.where(sv >= 0, sv << 1, ((-(sv + 1)) << 1) | 1).astype(U)
    sc_case = rc_._from_values(pat, np.zeros(sv.size, bool), None, nplanes=24, with_nn=False)
    ssc, _, _ = rc_.device_scanner(bm, ctx, sc_case)
    signed = bm.slice_scanner(ctx, ssc.slices, size=sv.size, signed=True)
    got = signed.values()
    assert got.dtype == np.int64 and np.array_equal(got, sv)
    assert np.array_equal(ssc.values().astype(U), pat)                    # the unsigned view: patterns
    with pytest.raises(bm.BmxError) as e:
        t.remap(None, signed)
    assert e.value.status == BADARG


_REDZONE_SCRIPT = r'''
import json, os, sys
sys.path.insert(0, os.getcwd())
sys.path.insert(0, os.path.join(os.getcwd(), "tests", "golden"))
import bitmagic_amd as bm
import remap_cases as rc_
fx = json.load(open(os.path.join("tests", "golden", "remap_ref.json")))["cases"]
ctx = bm.context(0)
out = {"enabled": ctx.redzone_check()["enabled"], "ok": True}
t = bm.set2set_11_transform(ctx)
for name in ("grid", "grid_planes", "sweep", "planes_64_image"):
    e = fx[name]
    sc, sel, vecs = rc_.device_scanner(bm, ctx, rc_.cases()[name])
    vals, rows = sc.values(sel, rows=True)
    img = t.remap(sel, sc)
    out["ok"] = (out["ok"] and rc_.sha(vals.astype("<u8")) == e["values_sha"] and rc_.sha(rows.astype("<u8")) == e["rows_sha"]
                 and rc_.sha(img.to_indices().astype("<u8")) == e["image_sha"] and t.n_rows == e["n_rows"])
    del img
ctx.synchronize()
out["hits"] = ctx.redzone_check()["hits"]
print("REDZONE " + json.dumps(out))
'''


def test_red_zones_clean():
    """a fresh process under BMX_DEBUG_REDZONE=1: the kind grids, the selected-rows sweep and 64 planes write nothing outside
    their allocations"""
    env = dict(os.environ, BMX_DEBUG_REDZONE="1")
    r = subprocess.run([sys.executable, "-c", _REDZONE_SCRIPT], capture_output=True, text=True, timeout=600, cwd=ROOT, env=env)
    line = [l for l in r.stdout.splitlines() if l.startswith("REDZONE ")]
    assert r.returncode == 0 and line, (r.stdout + r.stderr)[-3000:]
    out = json.loads(line[0][8:])
    assert out["enabled"] and out["hits"] == 0, out
    assert out["ok"], out
