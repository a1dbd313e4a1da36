"""GPU: the bit-sliced comparison search (bmx_slice_compare / bmx_slice_compare_signed, kernels k_slice_compare and
k_slice_compare_halves) and the scanner's equality family against the integer model of tests/golden/scanner_cmp_cases.py:
row i matches iff it is not NULL, i < size and the predicate holds in plain integer arithmetic.  test_scanner_model_host.py
ties that model to the reference's results and checks that the columns hold the block kinds planned for them; here every
operand is uploaded with exactly those kinds (the oracle port's block table), so the sign plane, the not-NULL vector and the
magnitude planes are NULL, FULL, GAP and bit-blocks, 64 planes wide, shorter than the column, absent.

At 64-bit width the expectation is the integer model and not the reference (include/bmx.h, bmx_slice_compare_signed)."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import bitmagic_amd as bm  # noqa: E402
from bitmagic_amd import _ffi  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import scanner_cmp_cases as sc  # noqa: E402
from cases import SCANNER_ROWS, s2u as fixture_s2u, scanner_values_signed, sha  # noqa: E402

B = sc.B
COLUMNS = sc.all_columns()
FORMS = ((True, True), (True, False), (False, True))          # (result, count): both, the vector only, the count only


def upload(ctx, port, bits):
    """a device vector of bits.size bits with the block kinds the oracle stores the content with"""
    nbits = int(bits.size)
    nblk = (nbits + B - 1) // B
    return bm.bvector.from_block_table(ctx, nbits, *port.import_words(sc.pack(bits, nblk * 2048), True, nbits).flatten())


class DeviceColumn:
    def __init__(self, ctx, port, col):
        pl, nn = col.operands()
        self.ctx, self.col = ctx, col
        self.planes = [None if p is None else upload(ctx, port, p) for p in pl]
        self.nn = None if nn is None else upload(ctx, port, nn)
        self.arr = (C.c_void_p * max(len(self.planes), 1))()
        for i, p in enumerate(self.planes):
            self.arr[i] = p._h if p is not None else None

    def raw(self, pred, v0=0, v1=0, size=None, want_result=True, want_count=True):
        """one call of the C entry -> (status, bvector or None, count)"""
        h, cnt = C.c_void_p(), C.c_uint64(12345)
        fn = bm.lib().bmx_slice_compare_signed if self.col.signed else bm.lib().bmx_slice_compare
        rc = fn(self.ctx._h, self.arr, len(self.planes), pred, v0, v1, self.col.size if size is None else size,
                self.nn._h if self.nn is not None else None, C.byref(h) if want_result else None, C.byref(cnt) if want_count else None)
        return rc, (bm.bvector(self.ctx, h) if h.value else None), cnt.value

    def scanner(self):
        return bm.slice_scanner(self.ctx, self.planes, size=self.col.size, not_null=self.nn, signed=self.col.signed)


@pytest.fixture(scope="module")
def device(ctx, port):
    """name -> DeviceColumn, uploaded once for the module"""
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = DeviceColumn(ctx, port, COLUMNS[name]())
        return cache[name]
    yield get
    cache.clear()


def check(dc, pred, v0=0, v1=0, size=None):
    """all three forms of the entry against the model: content as words, count() = the returned count = the model's, size()"""
    col = dc.col
    n = col.size if size is None else size
    exp = col.expect(pred, v0, v1, n)
    words, ecount = sc.pack(exp), int(exp.sum())
    what = (col.name, pred, v0, v1, n)
    for want_result, want_count in FORMS:
        rc, v, cnt = dc.raw(pred, v0, v1, size, want_result, want_count)
        assert rc == 0, what
        assert cnt == (ecount if want_count else 12345), (what, cnt, ecount)
        assert (v is not None) == want_result
        if v is not None:
            assert v.size() == n and v.count() == ecount, (what, v.size(), v.count(), ecount)
            got = v.to_words(words.size)
            assert (got == words).all(), (what, "first differing word", int(np.flatnonzero(got != words)[0]))
    return ecount


def run_column(ctx, dc, bounds, ranges):
    """every predicate at every bound, every range, zero and nonzero; both kernel shapes"""
    seen = set()
    try:
        for halves in (1, 0):
            ctx.set_tuning("range_halves", halves)
            for v in bounds:
                for pred in (sc.GT, sc.GE, sc.LT, sc.LE, sc.EQ):
                    seen.add(check(dc, pred, v) > 0)
            for lo, hi in ranges:
                check(dc, sc.RANGE, lo, hi)
            check(dc, sc.ZERO); check(dc, sc.NONZERO)
    finally:
        ctx.set_tuning("range_halves", 1)
    return seen


@pytest.mark.parametrize("name", sorted(COLUMNS))
def test_column_against_the_integer_model(ctx, device, name):
    dc = device(name)
    seen = run_column(ctx, dc, sc.bounds(dc.col), sc.ranges(dc.col))
    assert seen == {True, False}                                # some searches hit, some come back empty


def test_uploaded_operands_hold_the_planned_kinds(device):
    """what the host test reads from the oracle's block table is what the device holds"""
    kinds = {bm.NULL, bm.FULL, bm.GAP, bm.BIT}
    dc = device("kinds_signed64")
    assert {int(k) for k in dc.planes[0].block_table()[0]} == kinds and {int(k) for k in dc.nn.block_table()[0]} == kinds
    assert {int(k) for p in dc.planes[1:] for k in p.block_table()[0]} == kinds
    dc = device("kinds_signed64_nonull")
    plan = {0: bm.NULL, 1: bm.FULL, 2: bm.GAP, 3: bm.BIT}
    assert [int(k) for k in dc.planes[0].block_table()[0]] == [plan[b & 3] for b in range(16)]
    assert len(dc.planes) == 65 and dc.planes[64] is None
    dc = device("short_operands_signed")
    assert (dc.planes[0].info()["nblocks"], dc.nn.info()["nblocks"], dc.planes[5].info()["nblocks"], dc.planes[1].info()["nblocks"]) == (2, 3, 1, 6)


def _size_cases(col):
    if col.signed:
        return [(sc.GT, -5, 0), (sc.LT, 5, 0), (sc.LE, -1, 0), (sc.GE, 0, 0), (sc.NONZERO, 0, 0), (sc.ZERO, 0, 0), (sc.RANGE, -5, 5)]
    return [(sc.GT, 5, 0), (sc.LT, 5, 0), (sc.LE, 1, 0), (sc.GE, 0, 0), (sc.NONZERO, 0, 0), (sc.ZERO, 0, 0), (sc.RANGE, 0, 5)]


@pytest.mark.parametrize("name", ["kinds_signed64_nonull", "kinds_signed64", "kinds_unsigned64_nonull"])
def test_sizes(ctx, device, name):
    """size() below, at and beyond the planes' length: the sign modes that fill rows from the sign block alone (every row >= 0,
    every row < 0) leave nothing at or past size; rows past the planes' end hold 0 (and are NULL where there is a not-NULL vector)"""
    dc = device(name)
    own = dc.col.size
    sizes = [0, 1, 31, 32, 33, B - 1, B, B + 1, own, own - 70000, own + 2 * B]
    try:
        for halves in (1, 0):
            ctx.set_tuning("range_halves", halves)
            for size in sizes:
                for pred, v0, v1 in _size_cases(dc.col):
                    check(dc, pred, v0, v1, size)
    finally:
        ctx.set_tuning("range_halves", 1)
    if name == "kinds_signed64_nonull":                        # the cases are not vacuous: past the planes every row is a +0 without NULLs
        assert dc.col.expect(sc.GE, 0, 0, own + 2 * B)[own:].all() and dc.col.expect(sc.LT, 5, 0, own + 2 * B)[own:].all()
        assert dc.col.expect(sc.LE, -1, 0, own - 70000).any() and (dc.col.values[own - 70000:] < 0).any()


# ---- signed equality through the public facade ----------------------------------------------------------------------------------
def _first(bits):
    idx = np.flatnonzero(bits)
    return (True, int(idx[0])) if idx.size else (False, 0)


def _check_equality_family(s, values, valid, n, singles, lists, batch, methods):
    """find_eq / find_first_eq / find_eq_in / find_eq_indices / find_eq_counts of a signed scanner against the model"""
    nw = (n + 31) // 32
    model = lambda v: sc.expect(sc.EQ, v, 0, values, valid, n)
    for v in singles:
        e = model(v)
        t, found = s.find_eq(v)
        assert bool(found) == bool(e.any()), v
        assert (t is None and not e.any()) or (t.count() == int(e.sum()) and (t.to_words(nw) == sc.pack(e, nw)).all()), v
        if v != 0:                                              # (value 0 has no AND group: find_eq(0) covers it)
            f = s.find_first_eq(v)
            assert (bool(f[0]), int(f[1]) if f[0] else 0) == _first(e), (v, f)
        assert (s.find_eq_indices(v) == np.flatnonzero(e).astype(np.uint64)).all(), v
    for lst in lists:
        e = np.zeros(n, bool)
        for v in lst:
            e |= model(v)
        t = s.find_eq_in(lst)
        assert t.count() == int(e.sum()) and (t.to_words(nw) == sc.pack(e, nw)).all(), lst
    offsets, ids = s.find_eq_indices(batch)
    assert len(offsets) == len(batch) + 1 and int(offsets[-1]) == ids.size
    for q, v in enumerate(batch):
        assert (ids[int(offsets[q]):int(offsets[q + 1])] == np.flatnonzero(model(v)).astype(np.uint64)).all(), v
    for method in methods:
        got = s.find_eq_counts(batch, method=method)
        assert [int(x) for x in got] == [int(model(v).sum()) for v in batch], method


@pytest.mark.parametrize("with_null", [False, True])
def test_signed_equality_facade_int_fixture(ctx, golden, with_null):
    """the int column of the reference fixture: find_eq(v) and its family take SIGNED values (the reference maps the value with
    s2u first, src/bmsparsevec_algo.h:2603,2654) -- against golden["scanner"]["signed_*"]["cmp"]["eq"] and against the model"""
    g = golden["scanner"]["signed_with_null" if with_null else "signed_no_null"]
    n = SCANNER_ROWS
    nw = (n + 31) // 32
    vals, isn = scanner_values_signed(with_null)
    assert sha(vals) == g["values_sha"]
    u = fixture_s2u(vals)

    def up(bits):
        return bm.bit_import_u32(ctx, sc.pack(bits), True)
    planes = []
    for i in range(g["effective_slices"]):
        bits = ((u >> np.uint64(i)) & np.uint64(1)) != 0
        planes.append(up(bits) if bits.any() else None)
    s = bm.slice_scanner(ctx, planes, size=n, not_null=up(isn == 0) if with_null else None, signed=True)
    signs = set()
    for e in g["cmp"]["eq"]:
        t, found = s.find_eq(e["v"])
        assert bool(found) == (e["count"] > 0), e
        assert (t is None and e["count"] == 0) or (t.count() == e["count"] and sha(t.to_words(nw)) == e["sha"]), e
        if e["count"]:
            signs.add((e["v"] > 0) - (e["v"] < 0))
    assert signs == {-1, 0, 1}                                   # the fixture has hits on both sides of zero and at zero
    values, valid = vals.astype(np.int64), (None if isn is None else isn == 0)
    singles = [e["v"] for e in g["cmp"]["eq"]] + [5, -3, 1 << 40, -(1 << 40)]
    lists = [[0, -97, 1 << 40], [-1, 1, -70000, 70003], [1 << 40], [-2147483648, 2147483647, -2147483648], [0]]
    batch = [-97, 0, 5, 1 << 40, -1, 96, -2147483648, -3, 0]
    _check_equality_family(s, values, valid, n, singles, lists, batch, ("transpose", "pipeline", "auto"))
    # the unsigned container keeps its rule: a negative value is an argument error
    us = bm.slice_scanner(ctx, planes, size=n)
    with pytest.raises(bm.BmxError) as err:
        us.find_eq(-3)
    assert err.value.status == _ffi.ERR_BADARG
    with pytest.raises(bm.BmxError) as err:
        s.find_eq(1 << 63)
    assert err.value.status == _ffi.ERR_RANGE


@pytest.mark.parametrize("name", ["kinds_signed64", "kinds_signed64_nonull"])
def test_signed_equality_facade_64_planes(device, name):
    dc = device(name)
    col = dc.col
    present = sc.present_values(col)
    assert sc.I64_MIN in present and sc.I64_MAX in present
    singles = present + [0, 1, -1, sc.I64_MIN + 1, -2, 5, present[2] + 1, -(1 << 62) - 12345]
    lists = [[0, present[1], 1 << 62], [sc.I64_MIN, sc.I64_MAX, -1], [present[2] + 1]]
    batch = [present[1], 0, sc.I64_MIN, -1, present[2] + 1, sc.I64_MAX, 1]
    _check_equality_family(dc.scanner(), col.values, col.valid, col.size, singles, lists, batch, ("pipeline", "auto"))


# ---- argument errors ------------------------------------------------------------------------------------------------------------
def test_argument_errors_allocate_nothing(ctx, port, device):
    """every refusal comes back as a status before anything is allocated or launched: bmx_ctx_mem_used stays at its base"""
    L = bm.lib()
    sdc, udc = device("narrow_plane4_absent"), device("short_operands_unsigned")
    other = bm.context(0)
    foreign = upload(other, port, np.arange(3 * B) % 3 == 0)
    h, cnt = C.c_void_p(), C.c_uint64()

    def refused(rc, status=_ffi.ERR_BADARG):
        assert rc == status and h.value is None
        ctx.synchronize()
        assert ctx.mem_used() == base

    def call(dc, arr=None, n=None, pred=sc.GT, size=None, nn="own", res=True, count=True):
        fn = L.bmx_slice_compare_signed if dc.col.signed else L.bmx_slice_compare
        nnh = (dc.nn._h if dc.nn is not None else None) if nn == "own" else nn
        return fn(ctx._h, dc.arr if arr is None else arr, len(dc.planes) if n is None else n, pred, 1, 2,
                  dc.col.size if size is None else size, nnh, C.byref(h) if res else None, C.byref(cnt) if count else None)

    # the widest plane lists the entries take (all absent), and a warm-up whose results are gone before the base is read
    assert call(sdc, (C.c_void_p * 65)(), 65, res=False) == 0 and call(udc, (C.c_void_p * 64)(), 64, res=False) == 0
    assert sdc.raw(sc.GT, 1)[0] == 0 and udc.raw(sc.GT, 1)[0] == 0
    ctx.synchronize()
    base = ctx.mem_used()
    refused(call(sdc, (C.c_void_p * 66)(), 66))                              # 66 signed planes (sign + 64 is the most), 65 unsigned
    refused(call(udc, (C.c_void_p * 65)(), 65))
    for dc, pos in ((sdc, 0), (sdc, 3), (udc, 0), (udc, 3)):                 # a sign plane / a plane of another context
        arr = (C.c_void_p * len(dc.planes))(*[dc.arr[i] for i in range(len(dc.planes))])
        arr[pos] = foreign._h
        refused(call(dc, arr))
        refused(call(dc, arr, res=False))
    for dc in (sdc, udc):
        refused(call(dc, nn=foreign._h))                                     # ... as the not-NULL vector
        for pred in (-1, 8):
            refused(call(dc, pred=pred))
        refused(call(dc, res=False, count=False))                            # neither result nor count
        refused(call(dc, size=(1 << 36) + 1), _ffi.ERR_RANGE)                # more rows than a device vector has blocks for
        refused(call(dc, size=(1 << 36) + 1, res=False), _ffi.ERR_RANGE)
    # success: the result is the only thing that stays, and it goes with its handle
    rc, v, _ = sdc.raw(sc.GE, 0)
    ctx.synchronize()
    assert rc == 0 and ctx.mem_used() > base
    del v
    assert sdc.raw(sc.GE, 0, want_result=False)[0] == 0
    ctx.synchronize()
    assert ctx.mem_used() == base
    del foreign
    other.close()


# ---- red zones ------------------------------------------------------------------------------------------------------------------
_REDZONE_SCRIPT = r'''
import json, os, sys
sys.path.insert(0, os.getcwd())
sys.path.insert(0, os.path.join(os.getcwd(), "tests"))
sys.path.insert(0, os.path.join(os.getcwd(), "tests", "golden"))
import bitmagic_amd as bm
import oracle
import scanner_cmp_cases as sc
import test_gpu_scanner_compare as t
ctx = bm.context(0)
port = oracle.port()
out = {"enabled": ctx.redzone_check()["enabled"], "columns": 0}
for name in ("kinds_signed64", "kinds_signed64_nonull", "kinds_unsigned64", "short_operands_signed"):
    dc = t.DeviceColumn(ctx, port, t.COLUMNS[name]())
    lo, hi = dc.col.type_range()
    t.run_column(ctx, dc, [b for b in (lo, hi, 0, 1, -1, 5, -5) if lo <= b <= hi], sc.ranges(dc.col)[:6])
    own = dc.col.size
    for size in (1, 33, sc.B + 1, own - 70000, own + 2 * sc.B):
        for pred, v0, v1 in t._size_cases(dc.col):
            t.check(dc, pred, v0, v1, size)
    out["columns"] += 1
    del dc
ctx.synchronize()
out["hits"] = ctx.redzone_check()["hits"]
print("REDZONE " + json.dumps(out))
'''


def test_red_zones_clean():
    """a fresh process under BMX_DEBUG_REDZONE=1: the kind grids and the short operands, every form of the entry, both kernel
    shapes, sizes off the planes' length -- nothing is written outside an allocation (and every result equals the model)"""
    env = dict(os.environ, BMX_DEBUG_REDZONE="1")
    r = subprocess.run([sys.executable, "-c", _REDZONE_SCRIPT], capture_output=True, text=True, timeout=300, cwd=ROOT, env=env)
    line = [l for l in r.stdout.splitlines() if l.startswith("REDZONE ")]
    assert r.returncode == 0 and line, (r.stdout + r.stderr)[-3000:]
    out = json.loads(line[0][8:])
    assert out["enabled"] and out["hits"] == 0 and out["columns"] == 4, out
