"""GPU: which rows differ between two resident bit-sliced columns (bmx_slice_mismatch / bmx_slice_first_mismatch and the Python
facade over them) against sv_mismatch_ref.json -- the reference's sparse_vector_find_mismatch / sparse_vector_find_first_mismatch
(src/bmsparsevec_algo.h:656-792, 478-636) -- and against the NumPy model on the rows' values.  Content is compared by the hash of
the ascending positions; the result's block representation is the library's own (store_result's rule)."""
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
import sv_mismatch_cases as mc  # noqa: E402

B = 65536
BADARG = 2
with open(os.path.join(ROOT, "tests", "golden", "sv_mismatch_ref.json")) as _f:
    FX = json.load(_f)["cases"]


def _raw(ctx, a, b, proc, want_result=True, want_count=True):
    """one call of the C entry -> (status, bvector or None, count)"""
    h, cnt = C.c_void_p(), C.c_uint64(12345)
    rc = bm.lib().bmx_slice_mismatch(ctx._h, *bm._mismatch_args(a, b), proc, C.byref(h) if want_result else None, C.byref(cnt) if want_count else None)
    return rc, (bm.bvector(ctx, h) if h.value else None), cnt.value


def _raw_first(ctx, a, b, proc):
    found, idx = C.c_int(77), C.c_uint64(12345)
    rc = bm.lib().bmx_slice_first_mismatch(ctx._h, *bm._mismatch_args(a, b), proc, C.byref(found), C.byref(idx))
    return rc, [bool(found.value), idx.value]


def _check(ctx, case, exp):
    a, b = mc.device_scanners(bm, ctx, case)
    for pname, proc in mc.PROCS.items():
        e = exp[pname]
        rc, first = _raw_first(ctx, a, b, proc)
        assert rc == 0 and first == e["first"], (pname, first, e["first"])
        if e["count"] is None:                                # use_null without any not-NULL vector
            for wr, wc in ((True, True), (True, False), (False, True)):
                rc, v, _ = _raw(ctx, a, b, proc, wr, wc)
                assert rc == BADARG and v is None and b"id_max" in bm.lib().bmx_last_error()
            continue
        rc, v, cnt = _raw(ctx, a, b, proc)
        assert rc == 0 and cnt == e["count"], (pname, cnt, e["count"])
        ids = v.to_indices()
        assert ids.size == e["count"] and mc.sha(ids.astype("<u8")) == e["ids_sha"], pname
        assert v.size() == exp["size"] and v.count() == e["count"]
        rc, v2, cnt = _raw(ctx, a, b, proc, want_count=False)
        assert rc == 0 and cnt == 12345 and mc.sha(v2.to_indices().astype("<u8")) == e["ids_sha"]
        rc, none, cnt = _raw(ctx, a, b, proc, want_result=False)         # count only: nothing is materialised
        assert rc == 0 and none is None and cnt == e["count"], (pname, cnt)


@pytest.mark.parametrize("name", sorted(FX))
def test_fixture_case(ctx, name):
    _check(ctx, mc.cases()[name], FX[name])


def test_result_blocks_follow_the_storage_rule(ctx):
    """all rows differ: FULL blocks and a partial tail (one run: a GAP block); equal content: nothing but NULL blocks"""
    a, b = mc.device_scanners(bm, ctx, mc.cases()["all_rows_differ"])
    v = bm.sparse_vector_find_mismatch(a, b, bm.NO_NULL)
    kinds = v.block_table()[0]
    assert list(kinds) == [bm.FULL, bm.FULL, bm.GAP]
    a, b = mc.device_scanners(bm, ctx, mc.cases()["equal_gap_vs_bit"])
    assert {int(k) for k in a.slices[0].block_table()[0]} == {bm.GAP} and {int(k) for k in b.slices[0].block_table()[0]} == {bm.BIT}
    v = bm.sparse_vector_find_mismatch(a, b, bm.USE_NULL)
    assert list(v.block_table()[0]) == [bm.NULL] * 3
    g = mc.cases()["grid"]                                   # the grid's operands hold the kinds the case was planned with
    gv = mc.device_vecs(bm, ctx, g)
    plan = {0: bm.NULL, 1: bm.FULL, 2: bm.GAP, 3: bm.BIT}
    for key, shift in (("a0", 0), ("b0", 2), ("a1", 2), ("b1", 0)):
        kinds = gv[key].block_table()[0]
        assert [int(k) for k in kinds[:15]] == [plan[(c >> shift) & 3] for c in range(15)], key


def test_python_facade(ctx):
    for name in ("grid_nn", "ragged_5_9", "size_across_only_a", "five_rows", "no_planes"):
        case, exp = mc.cases()[name], FX[name]
        a, b = mc.device_scanners(bm, ctx, case)
        for pname, proc in mc.PROCS.items():
            v = bm.sparse_vector_find_mismatch(a, b, proc)
            assert isinstance(v, bm.bvector) and mc.sha(v.to_indices().astype("<u8")) == exp[pname]["ids_sha"]
            assert bm.sparse_vector_count_mismatch(a, b, proc) == exp[pname]["count"]
            assert list(bm.sparse_vector_find_first_mismatch(a, b, proc)) == exp[pname]["first"]
        assert list(bm.sparse_vector_find_first_mismatch(a, b)) == exp["use_null"]["first"]        # the default is use_null
    a, b = mc.device_scanners(bm, ctx, mc.cases()["grid"])
    with pytest.raises(bm.BmxError) as e:
        bm.sparse_vector_find_mismatch(a, b, bm.USE_NULL)
    assert e.value.status == BADARG and "id_max" in str(e.value)
    # two signed columns compare as they are (the sign is plane 0); one signed against one unsigned is refused
    sa = bm.slice_scanner(ctx, a.slices, size=a.size(), signed=True)
    sb = bm.slice_scanner(ctx, b.slices, size=b.size(), signed=True)
    assert bm.sparse_vector_count_mismatch(sa, sb, bm.NO_NULL) == FX["grid"]["no_null"]["count"]
    for f in (lambda: bm.sparse_vector_find_mismatch(sa, b, bm.NO_NULL), lambda: bm.sparse_vector_count_mismatch(a, sb, bm.NO_NULL),
              lambda: bm.sparse_vector_find_first_mismatch(sa, b)):
        with pytest.raises(bm.BmxError) as e:
            f()
        assert e.value.status == BADARG


@pytest.mark.parametrize("window", [0, 1, -1])
def test_first_mismatch_windows(ctx, window):
    """the difference in the last of 40 block columns: the default windows, one column per launch, one launch for all"""
    try:
        ctx.set_tuning("ff_window", window)
        for name in ("first_in_last_of_40_columns", "first_at_row0", "grid_nn", "same_handles"):
            a, b = mc.device_scanners(bm, ctx, mc.cases()[name])
            for pname, proc in mc.PROCS.items():
                assert list(bm.sparse_vector_find_first_mismatch(a, b, proc)) == FX[name][pname]["first"], (name, pname)
    finally:
        ctx.set_tuning("ff_window", 0)


def _random_case(seed: int):
    rng = np.random.default_rng(seed)
    sa, sb = (int(rng.integers(1, 3 * B)) for _ in range(2))
    if seed % 3 == 0:
        sb = sa
    vecs, cols = {}, []
    for side, size in (("a", sa), ("b", sb)):
        nblk = (size + B - 1) // B
        planes = []
        for i in range(int(rng.integers(1, 7))):
            if rng.random() < 0.15:
                planes.append(None); continue
            k = "%s%d" % (side, i)
            vecs[k] = mc._cut(mc._mixed(seed * 100 + i + (50 if side == "b" and rng.random() < 0.5 else 0), nblk), size)
            planes.append(k)
        nn = None
        if rng.random() < 0.7:
            nn = "n" + side
            vecs[nn] = mc._cut(mc._mixed(seed * 100 + 90 + (side == "b"), nblk), size)
        cols.append(mc._col(planes, size, nn))
    return mc._case(vecs, cols[0], cols[1])


@pytest.mark.parametrize("seed", range(12))
def test_random_columns_against_the_value_model(ctx, seed):
    case = _random_case(1000 + seed)
    _check(ctx, case, mc.model_case(case))


def test_bad_arguments_and_no_leak(ctx):
    """every refusal of the two entries, and bmx_ctx_mem_used back at its base after each of them and after success"""
    case = mc.cases()["grid_nn"]
    a, b = mc.device_scanners(bm, ctx, case)
    plain_a, plain_b = mc.device_scanners(bm, ctx, mc.cases()["grid"])
    other = bm.context(0)
    foreign = bm.bit_import_u32(other, mc.case_words(case, "a0"), True)
    L = bm.lib()
    args = bm._mismatch_args(a, b)
    h, cnt, found, idx = C.c_void_p(), C.c_uint64(), C.c_int(), C.c_uint64()
    vec = lambda *ar: L.bmx_slice_mismatch(ctx._h, *ar, C.byref(h), C.byref(cnt))
    first = lambda *ar: L.bmx_slice_first_mismatch(ctx._h, *ar, C.byref(found), C.byref(idx))
    many = (C.c_void_p * 66)()
    assert vec(*args, bm.NO_NULL) == 0 and first(*args, bm.NO_NULL) == 0
    warm = bm.bvector(ctx, h)                                # (the warm-up result goes before the base is read)
    del warm
    h = C.c_void_p()
    ctx.synchronize()
    base = ctx.mem_used()

    def refused(rc):
        assert rc == BADARG and h.value is None
        ctx.synchronize()
        assert ctx.mem_used() == base

    refused(L.bmx_slice_mismatch(None, *args, bm.NO_NULL, C.byref(h), C.byref(cnt)))                      # null context
    refused(L.bmx_slice_first_mismatch(None, *args, bm.NO_NULL, C.byref(found), C.byref(idx)))
    for pos in (0, 4):                                                                                    # a vector of another context
        bad = list(args)
        arr = (C.c_void_p * 2)(); arr[0] = foreign._h; arr[1] = args[pos][1]
        bad[pos] = arr
        refused(vec(*bad, bm.NO_NULL)); refused(first(*bad, bm.NO_NULL))
    for pos in (3, 7):                                                                                    # ... as a not-NULL vector
        bad = list(args); bad[pos] = foreign._h
        refused(vec(*bad, bm.NO_NULL)); refused(first(*bad, bm.USE_NULL))
    for pos in (0, 4):                                                                                    # more than 65 planes
        bad = list(args); bad[pos] = many; bad[pos + 1] = 66
        refused(vec(*bad, bm.NO_NULL)); refused(first(*bad, bm.NO_NULL))
    ok65 = list(args); ok65[0] = many; ok65[1] = 65                                                       # 65 (absent) planes are allowed
    assert first(*ok65, bm.NO_NULL) == 0
    for proc in (2, -1):                                                                                  # an unknown null_proc
        refused(vec(*args, proc)); refused(first(*args, proc))
    refused(L.bmx_slice_mismatch(ctx._h, *args, bm.NO_NULL, None, None))                                  # neither result nor count
    refused(L.bmx_slice_first_mismatch(ctx._h, *args, bm.NO_NULL, None, C.byref(idx)))
    refused(L.bmx_slice_first_mismatch(ctx._h, *args, bm.NO_NULL, C.byref(found), None))
    refused(vec(*bm._mismatch_args(plain_a, plain_b), bm.USE_NULL))                                       # use_null, no not-NULL vector
    refused(L.bmx_slice_mismatch(ctx._h, *bm._mismatch_args(plain_a, plain_b), bm.USE_NULL, None, C.byref(cnt)))
    # success: the result is the only thing that stays, and it goes with its handle
    for proc in (bm.USE_NULL, bm.NO_NULL):
        v = bm.sparse_vector_find_mismatch(a, b, proc)
        ctx.synchronize()
        assert ctx.mem_used() > base
        del v
        assert bm.sparse_vector_count_mismatch(a, b, proc) == FX["grid_nn"][mc_name(proc)]["count"]
        assert list(bm.sparse_vector_find_first_mismatch(a, b, proc)) == FX["grid_nn"][mc_name(proc)]["first"]
        ctx.synchronize()
        assert ctx.mem_used() == base
    del foreign
    other.close()


def mc_name(proc):
    return "use_null" if proc == bm.USE_NULL else "no_null"


_REDZONE_SCRIPT = r'''
import json, os, sys
sys.path.insert(0, os.getcwd())
sys.path.insert(0, os.path.join(os.getcwd(), "tests", "golden"))
import bitmagic_amd as bm
import sv_mismatch_cases as mc
fx = json.load(open(os.path.join("tests", "golden", "sv_mismatch_ref.json")))["cases"]
ctx = bm.context(0)
out = {"enabled": ctx.redzone_check()["enabled"], "ok": True}
for name in ("grid", "grid_nn", "size_across_both", "planes_64"):
    a, b = mc.device_scanners(bm, ctx, mc.cases()[name])
    for pname, proc in mc.PROCS.items():
        e = fx[name][pname]
        if e["count"] is not None:
            v = bm.sparse_vector_find_mismatch(a, b, proc)
            out["ok"] = out["ok"] and mc.sha(v.to_indices().astype("<u8")) == e["ids_sha"] and bm.sparse_vector_count_mismatch(a, b, proc) == e["count"]
            del v
        for w in (0, 1, -1):
            ctx.set_tuning("ff_window", w)
            out["ok"] = out["ok"] and list(bm.sparse_vector_find_first_mismatch(a, b, proc)) == e["first"]
        ctx.set_tuning("ff_window", 0)
ctx.synchronize()
out["hits"] = ctx.redzone_check()["hits"]
print("REDZONE " + json.dumps(out))
'''


def test_red_zones_clean():
    """a fresh process under BMX_DEBUG_REDZONE=1: the grids, a size difference across blocks and 64 planes, all three endings,
    write nothing outside their allocations"""
    env = dict(os.environ, BMX_DEBUG_REDZONE="1")
    r = subprocess.run([sys.executable, "-c", _REDZONE_SCRIPT], capture_output=True, text=True, timeout=600, cwd=ROOT, env=env)
    line = [l for l in r.stdout.splitlines() if l.startswith("REDZONE ")]
    assert r.returncode == 0 and line, (r.stdout + r.stderr)[-3000:]
    out = json.loads(line[0][8:])
    assert out["enabled"] and out["hits"] == 0, out
    assert out["ok"], out
