"""GPU: batched range counts over resident bit-sliced columns (bmx_slice_range_counts / _signed / bmx_gslice_range_counts, kernel
k_slice_le_counts, and slice_scanner.find_range_counts / histogram over them) against the integer model of
tests/golden/scanner_cmp_cases.py: counts[q] = Column.expect(RANGE, lo[q], hi[q]).sum().  test_scanner_model_host.py ties that
model to the reference's find_range results.  Every operand is uploaded with the block kinds the oracle stores it with, as
test_gpu_scanner_compare.py does."""
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

B = sc.B
COLUMNS = sc.all_columns()
T = _ffi.RC_BATCH_MAX
POISON = 0xDEADBEEFCAFEF00D


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

    def raw(self, lo, hi, size=None, out=None):
        """one call of the C entry -> (status, counts)"""
        dt = np.int64 if self.col.signed else np.uint64
        lo, hi = np.array([int(v) for v in lo], dt), np.array([int(v) for v in hi], dt)
        out = np.full(lo.size, POISON, np.uint64) if out is None else out
        fn = bm.lib().bmx_slice_range_counts_signed if self.col.signed else bm.lib().bmx_slice_range_counts
        rc = fn(self.ctx._h, self.arr, len(self.planes), lo.ctypes.data_as(C.c_void_p), hi.ctypes.data_as(C.c_void_p), lo.size,
                self.col.size if size is None else size, self.nn._h if self.nn is not None else None, out.ctypes.data_as(C.c_void_p))
        return rc, out

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


def model(col, ranges, size=None):
    return np.array([int(col.expect(sc.RANGE, lo, hi, size).sum()) for lo, hi in ranges], np.uint64)


def check(dc, ranges, size=None, exp=None):
    exp = model(dc.col, ranges, size) if exp is None else exp
    rc, got = dc.raw([r[0] for r in ranges], [r[1] for r in ranges], size)
    assert rc == 0, (dc.col.name, bm.lib().bmx_last_error())
    bad = np.flatnonzero(got != exp)
    assert bad.size == 0, (dc.col.name, size, [(ranges[i], int(got[i]), int(exp[i])) for i in bad[:5]])
    return exp


def column_ranges(col):
    """ranges(col) plus (b, b) and (type_min, b) for every bound of the column"""
    tmin = col.type_range()[0]
    bs = sc.bounds(col)
    return sc.ranges(col) + [(b, b) for b in bs] + [(tmin, b) for b in bs]


# ---- 1. every column against the model, and against the loop of bmx_slice_compare calls -------------------------------------------
def run_column(ctx, dc):
    ranges = column_ranges(dc.col)
    exp = check(dc, ranges)
    try:
        ctx.set_tuning("rc_batch", -1)
        check(dc, ranges, exp=exp)
    finally:
        ctx.set_tuning("rc_batch", 0)
    return exp


@pytest.mark.parametrize("name", sorted(COLUMNS))
def test_column_against_the_integer_model(ctx, device, name):
    exp = run_column(ctx, device(name))
    assert (exp > 0).any()                                      # the case is not vacuous: some ranges hit


# ---- 2. pass boundaries -----------------------------------------------------------------------------------------------------------
def threshold_ranges(col, k, seed):
    """ranges whose distinct thresholds are exactly k values t[0] < .. < t[k-1] below every plane's top: [0, t0], then the
    magnitude intervals [t[i] + 1, t[i+1]] -- on the negative side for every other one of a signed column"""
    rng = np.random.default_rng(seed)
    t = sorted(int(x) for x in rng.choice(2040, k, replace=False))
    t[-1] += (1 << 40) + 7                                       # one wide threshold: the high planes take part
    out = [(0, t[0])]
    for i in range(k - 1):
        a, b = t[i] + 1, t[i + 1]
        out.append((-b - 1, -a - 1) if col.signed and i % 2 else (a, b))
    return out


def run_pass_boundaries(ctx, dc):
    try:
        for batch in (1, 3, 0):
            ctx.set_tuning("rc_batch", batch)
            per = batch or T
            for k in (per - 1, per, per + 1, 2 * per + 1):
                if k < 1:
                    continue
                ranges = threshold_ranges(dc.col, k, 100 * per + k)
                exp = check(dc, ranges)
                check(dc, ranges[::-1], exp=exp[::-1])
                check(dc, [r for r in ranges for _ in (0, 1)], exp=np.repeat(exp, 2))
    finally:
        ctx.set_tuning("rc_batch", 0)


@pytest.mark.parametrize("name", ["kinds_unsigned64", "kinds_signed64"])
def test_pass_boundaries(ctx, device, name):
    run_pass_boundaries(ctx, device(name))


# ---- 3. edges ---------------------------------------------------------------------------------------------------------------------
def test_no_ranges_writes_nothing(device):
    for name in ("kinds_unsigned64", "kinds_signed64"):
        dc = device(name)
        out = np.full(4, POISON, np.uint64)
        dt = np.int64 if dc.col.signed else np.uint64
        fn = bm.lib().bmx_slice_range_counts_signed if dc.col.signed else bm.lib().bmx_slice_range_counts
        some = np.zeros(1, dt)
        nn = dc.nn._h if dc.nn is not None else None
        for lo, hi, cnt in ((some, some, out), (None, None, None)):
            p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
            assert fn(dc.ctx._h, dc.arr, len(dc.planes), p(lo), p(hi), 0, dc.col.size, nn, p(cnt)) == 0
        assert (out == POISON).all()


@pytest.mark.parametrize("name", ["kinds_unsigned64", "kinds_signed64", "kinds_signed64_nonull", "short_operands_signed", "narrow_plane4_absent"])
def test_sizes(device, name):
    dc = device(name)
    ranges = sc.ranges(dc.col)
    for size in (0, 1, 65535, 65536, 65537, dc.col.size - 1):
        exp = check(dc, ranges, size)
        assert size > 0 or not exp.any()


@pytest.mark.parametrize("name", sorted(COLUMNS))
def test_reversed_and_extreme_ranges(device, name):
    dc = device(name)
    col = dc.col
    tmin, tmax = col.type_range()
    check(dc, [(hi, lo) for lo, hi in column_ranges(col)[:40]])                     # all ranges reversed
    extremes = [(0, 0), (0, 5), (0, tmax), (tmin, tmax), (tmin, tmin), (tmax, tmax), (tmax - 1, tmax)]
    if col.signed:
        extremes += [(sc.I64_MIN, sc.I64_MAX), (sc.I64_MIN, sc.I64_MIN), (-1, 0), (sc.I64_MIN, -1), (sc.I64_MIN + 1, 0)]
    else:
        extremes += [(0, sc.U64_MAX), (1, sc.U64_MAX), (sc.U64_MAX, sc.U64_MAX), (1 << 63, sc.U64_MAX)]
    check(dc, extremes)
    if col.nplanes < 41:                                                            # bounds with bits above every plane
        mm = sc.max_magnitude(col)
        wide = [(0, 1 << 40), (1 << 40, 1 << 41), (mm, 1 << 40), (mm + 1, 1 << 40), (3, (1 << 40) + 3)]
        if col.signed:
            wide += [(-(1 << 40), 1 << 40), (-(1 << 41), -(1 << 40)), (-(1 << 40), -1), (-(1 << 40) - 3, -(mm + 1)), (-(mm + 2), 0)]
        check(dc, wide)


@pytest.mark.parametrize("signed", [True, False])
def test_thousand_random_ranges(device, signed):
    dc = device("short_operands_signed" if signed else "short_operands_unsigned")
    rng = np.random.default_rng(64100 + signed)
    lo = rng.integers(-3000 if signed else 0, 5000, 1000)
    hi = lo + rng.integers(-50, 1500, 1000)                                        # (some reversed)
    if not signed:
        hi = np.maximum(hi, 0)
    check(dc, list(zip((int(x) for x in lo), (int(x) for x in hi))))


# ---- 4. histogram -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["kinds_unsigned64", "kinds_signed64", "kinds_signed64_nonull", "narrow_plane4_absent", "narrow_no_planes",
                                  "short_operands_signed", "short_operands_unsigned_nonull"])
def test_histogram(device, name):
    dc = device(name)
    col, s = dc.col, dc.scanner()
    edges = sc.bounds(col)
    assert edges == sorted(set(edges)) and len(edges) > 8
    got = s.histogram(edges)
    assert got.dtype == np.uint64 and got.size == len(edges) - 1
    exp = model(col, [(a, b - 1) for a, b in zip(edges, edges[1:])])
    assert (got == exp).all(), (name, got, exp)
    assert int(got.sum()) == int(col.expect(sc.RANGE, edges[0], edges[-1] - 1).sum()) and got.any()
    twice = [e for e in edges for _ in (0, 1)]                                      # repeated edges: empty bins in between
    got2 = s.histogram(twice)
    assert (got2[1::2] == exp).all() and not got2[0::2].any()
    assert s.histogram([]).size == 0 and s.histogram(edges[:1]).size == 0
    with pytest.raises(bm.BmxError) as err:
        s.histogram([5, 3])
    assert err.value.status == _ffi.ERR_BADARG
    ranges = sc.ranges(col)
    got = s.find_range_counts([r[0] for r in ranges], [r[1] for r in ranges])
    assert got.dtype == np.uint64 and (got == model(col, ranges)).all()
    tmin, tmax = col.type_range()
    for lo, hi in (([tmin - 1], [0]), ([0], [tmax + 1])):                           # bounds outside the container's type
        with pytest.raises(bm.BmxError) as err:
            s.find_range_counts(lo, hi)
        assert err.value.status == _ffi.ERR_RANGE


# ---- 5. refusals and leaks --------------------------------------------------------------------------------------------------------
def test_bad_arguments_and_no_leak(ctx, port, device):
    """every refusal of the three entries, and bmx_ctx_mem_used back at its base after each of them and after success"""
    L = bm.lib()
    sdc, udc = device("narrow_plane4_absent"), device("short_operands_unsigned")
    other = bm.context(0)
    foreign = upload(other, port, np.arange(3 * B) % 3 == 0)
    lo, hi, out = np.array([1, 2], np.uint64), np.array([5, 9], np.uint64), np.full(2, POISON, np.uint64)
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)

    def call(dc, h="own", arr=None, n=None, size=None, nn="own", a=lo, b=hi, c=out, nr=2):
        fn = L.bmx_slice_range_counts_signed if dc.col.signed else L.bmx_slice_range_counts
        nnh = (dc.nn._h if dc.nn is not None else None) if nn == "own" else nn
        return fn(ctx._h if h == "own" else h, dc.arr if arr is None else arr, len(dc.planes) if n is None else n, p(a), p(b), nr,
                  dc.col.size if size is None else size, nnh, p(c))

    # the widest plane lists the entries take (all absent), and a warm-up before the base is read
    assert call(sdc, arr=(C.c_void_p * 65)(), n=65) == 0 and call(udc, arr=(C.c_void_p * 64)(), n=64) == 0
    assert call(sdc) == 0 and call(udc) == 0
    ctx.synchronize()
    base = ctx.mem_used()

    def refused(rc, status=_ffi.ERR_BADARG):
        assert rc == status
        ctx.synchronize()
        assert ctx.mem_used() == base

    for batch in (0, -1):                                                           # the batch path and the loop path refuse alike
        ctx.set_tuning("rc_batch", batch)
        try:
            for dc in (sdc, udc):
                out[:] = POISON
                refused(call(dc, h=None))                                           # null context
                assert (out == POISON).all()
                refused(call(dc, arr=(C.c_void_p * 66)(), n=66 if dc.col.signed else 65))   # more planes than bmx_slice_compare takes
                for pos in (0, 3):                                                  # a (sign) plane of another context
                    arr = (C.c_void_p * len(dc.planes))(*[dc.arr[i] for i in range(len(dc.planes))])
                    arr[pos] = foreign._h
                    refused(call(dc, arr=arr))
                refused(call(dc, nn=foreign._h))                                    # ... as the not-NULL vector
                refused(call(dc, a=None)); refused(call(dc, b=None)); refused(call(dc, c=None))   # lo / hi / counts NULL with n > 0
                refused(call(dc, size=(1 << 36) + 1), _ffi.ERR_RANGE)               # more rows than a device vector has blocks for
                assert call(dc) == 0 and (out == model(dc.col, [(1, 5), (2, 9)])).all()
                ctx.synchronize()
                assert ctx.mem_used() == base
        finally:
            ctx.set_tuning("rc_batch", 0)
    for bad in (-2, T + 1):                                                         # the tuning key checks its range
        with pytest.raises(bm.BmxError):
            ctx.set_tuning("rc_batch", bad)
    # the group entry
    grp = bm.group([0])
    gother = bm.group([0])
    bits = np.arange(3 * B) % 5 == 0
    tab = port.import_words(sc.pack(bits, 3 * 2048), True, 3 * B).flatten()
    gp, gf = bm.gbvector.from_block_table(grp, 3 * B, *tab), bm.gbvector.from_block_table(gother, 3 * B, *tab)
    gshort = bm.gbvector.from_block_table(grp, 2 * B, *port.import_words(sc.pack(bits[:2 * B], 2 * 2048), True, 2 * B).flatten())
    garr = (C.c_void_p * 2)(gp._h, gp._h)

    def gcall(g=grp, arr=garr, n=2, size=3 * B, nn=None, a=lo, b=hi, c=out, nr=2):
        return L.bmx_gslice_range_counts(g._h if g is not None else None, arr, n, p(a), p(b), nr, size, nn, p(c))

    assert gcall() == 0
    assert gcall(g=None) == _ffi.ERR_BADARG
    assert gcall(arr=(C.c_void_p * 65)(), n=65) == _ffi.ERR_BADARG
    assert gcall(arr=(C.c_void_p * 2)(gp._h, gf._h)) == _ffi.ERR_BADARG             # a plane of another group
    assert gcall(nn=gf._h) == _ffi.ERR_BADARG
    assert gcall(arr=(C.c_void_p * 2)(gp._h, gshort._h)) == _ffi.ERR_BADARG         # planes of different block ranges
    assert gcall(size=2 * B) == _ffi.ERR_BADARG                                     # size outside the planes' block range
    assert gcall(a=None) == _ffi.ERR_BADARG and gcall(b=None) == _ffi.ERR_BADARG and gcall(c=None) == _ffi.ERR_BADARG
    out[:] = POISON
    assert gcall(nr=0, a=None, b=None, c=None) == 0 and gcall(nr=0) == 0 and (out == POISON).all()
    v = np.where(bits, 3, 0)
    assert gcall() == 0 and [int(x) for x in out] == [int(((v >= 1) & (v <= 5)).sum()), int(((v >= 2) & (v <= 9)).sum())]
    del gp, gf, gshort, foreign
    grp.close(); gother.close(); other.close()


# ---- 6. red zones -----------------------------------------------------------------------------------------------------------------
_REDZONE_SCRIPT = r'''
import json, os, sys
sys.path.insert(0, os.getcwd())
sys.path.insert(0, os.path.join(os.getcwd(), "tests"))
sys.path.insert(0, os.path.join(os.getcwd(), "tests", "golden"))
import bitmagic_amd as bm
import oracle
import test_gpu_range_counts as t
ctx = bm.context(0)
port = oracle.port()
out = {"enabled": ctx.redzone_check()["enabled"], "columns": 0}
for name in ("kinds_signed64", "kinds_unsigned64", "short_operands_signed"):
    dc = t.DeviceColumn(ctx, port, t.COLUMNS[name]())
    t.run_column(ctx, dc)
    t.run_pass_boundaries(ctx, dc)
    out["columns"] += 1
    del dc
ctx.synchronize()
out["hits"] = ctx.redzone_check()["hits"]
print("REDZONE " + json.dumps(out))
'''


def test_red_zones_clean():
    """a fresh process under BMX_DEBUG_REDZONE=1: the two 64-plane grids and the short operands, the batch kernel at every pass
    boundary and the loop path -- nothing is written outside an allocation (and every count equals the model)"""
    env = dict(os.environ, BMX_DEBUG_REDZONE="1")
    r = subprocess.run([sys.executable, "-c", _REDZONE_SCRIPT], capture_output=True, text=True, timeout=300, cwd=ROOT, env=env)
    line = [l for l in r.stdout.splitlines() if l.startswith("REDZONE ")]
    assert r.returncode == 0 and line, (r.stdout + r.stderr)[-3000:]
    out = json.loads(line[0][8:])
    assert out["enabled"] and out["hits"] == 0 and out["columns"] == 3, out


# ---- 7. group ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("members", [1, 3, 8])
def test_group_counts_equal_the_single_device(ctx, port, device, members):
    dc = device("kinds_unsigned64")
    col = dc.col
    pl, nn = col.operands()
    grp = bm.group([0] * members)
    nblk = (col.size + B - 1) // B

    def gup(bits):
        return bm.gbvector.from_block_table(grp, col.size, *port.import_words(sc.pack(bits, nblk * 2048), True, col.size).flatten())
    gs = [None if p is None else gup(p) for p in pl]
    gsc = bm.gslice_scanner(grp, gs, size=col.size, not_null=gup(nn))
    ranges = column_ranges(col) + threshold_ranges(col, 2 * T + 1, 7)
    lo, hi = [r[0] for r in ranges], [r[1] for r in ranges]
    got = gsc.find_range_counts(lo, hi)
    assert (got == dc.scanner().find_range_counts(lo, hi)).all() and (got == model(col, ranges)).all()
    edges = sc.bounds(col)
    assert (gsc.histogram(edges) == dc.scanner().histogram(edges)).all()
    with pytest.raises(bm.BmxError) as err:
        gsc.find_range_counts([-1], [5])
    assert err.value.status == _ffi.ERR_RANGE
    del gsc, gs
    grp.close()
