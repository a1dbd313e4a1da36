"""GPU: pipeline results as index lists (bmx_pipeline_run_indices[_dev], aggregator.combine_and_sub_indices, slice_scanner.
find_eq_indices over a batch): every arg-group's hits as ascending positions in one CSR, against the oracle port's
agg_and_sub(and, sub).to_words() per group (and the reference's where it is built).  offsets and ids are compared for equality."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import bitmagic_amd as bm  # noqa: E402
import oracle  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import pipe_indices_cases as pc  # noqa: E402

B = 65536
RANGE = 3
U64P = C.POINTER(C.c_uint64)


@pytest.fixture(scope="module")
def grid(ctx, port):
    """operands on both sides, the kinds-grid pipeline and its expected CSR: built once, never modified"""
    pv = pc.oracle_operands(port)
    gv = pc.device_operands(bm, ctx, pv)
    groups = pc.grid_groups()
    off, ids = pc.expected_csr(port, pv, groups)
    off.setflags(write=False); ids.setflags(write=False)
    return {"pv": pv, "gv": gv, "groups": groups, "pipe": pc.make_pipeline(bm, ctx, gv, groups), "offsets": off, "ids": ids}


def _same(got, exp):
    assert got[0].dtype == np.uint64 and got[0].shape == exp[0].shape and (got[0] == exp[0]).all()
    assert got[1].shape == exp[1].shape and (got[1].astype(np.uint64) == exp[1]).all()


def _raw(ctx, pipe, nb_from, nb_to, width, cap, fill=0xAB):
    """one call of the C entry with a poisoned buffer of max(cap, 1) entries -> (status, n, offsets, buffer)"""
    offsets = np.full(pipe.size() + 1, 0x77, np.uint64)
    out = np.full(max(cap, 1), fill, np.uint64 if width == 8 else np.uint32)
    n = C.c_uint64(12345)
    rc = bm.lib().bmx_pipeline_run_indices(ctx._h, pipe._h, nb_from, nb_to, width, offsets.ctypes.data_as(U64P), bm._ptr(out), cap, C.byref(n))
    return rc, n.value, offsets, out


def test_kinds_grid(ctx, port, grid):
    """7 columns whose operands cycle through NULL / FULL / BIT / GAP; AND lists of 1 .. 17, SUB lists of 0 .. 5, ROW_FULL, GAP-only
    groups, empty AND lists, a disjoint pair, repeated operands, the same vector on both sides"""
    planned = {(k, c): pc.kinds_of(k[0], k[1], c) for k in pc.OPERANDS if k[0] != "d" for c in range(pc.NCOLS - 1)}
    for (k, c), kind in planned.items():                     # the device vectors hold the kinds the cases were planned with
        assert grid["gv"][k].block_table()[0][c] == kind, (k, c)
    assert {kind for kind in planned.values()} == {pc.NULL, pc.FULL, pc.BIT, pc.GAP}
    exp = (grid["offsets"], grid["ids"])
    sizes = np.diff(exp[0].astype(np.int64))
    assert sorted({len(a) for a, _ in grid["groups"]} & {1, 2, 3, 4, 5, 8, 9, 17}) == [1, 2, 3, 4, 5, 8, 9, 17]
    assert {len(s) for _, s in grid["groups"]} >= {0, 1, 2, 3, 4, 5}
    assert sizes[10] >= 2 * B and sizes[14] == 0 and sizes[15] == 0 and sizes[16] == 0 and sizes[18] == 0 and sizes[12] > 0
    assert (sizes > 0).sum() >= 15
    _same(bm.aggregator(ctx).combine_and_sub_indices(grid["pipe"]), exp)
    for unroll in (1, 2, 0):                                 # every operand-fold batch size of the kernels
        ctx.set_tuning("pipe_unroll", unroll)
        _same(bm.aggregator(ctx).combine_and_sub_indices(grid["pipe"]), exp)
    if oracle.have_reference("avx2"):
        R = oracle.reference("avx2")
        _same(pc.expected_csr(R, pc.oracle_operands(R), grid["groups"]), exp)


def test_ragged_lengths(ctx, port):
    """operands of 3, 7 and 12 blocks in one group: columns beyond an AND operand's end are empty, beyond a SUB operand's untouched"""
    n3, n7, n12 = 3 * B - 5, 7 * B - 77, 11 * B + 9
    keys = {("a", 6): n12, ("a", 7): n7, ("a", 8): n3, ("s", 1): n3, ("s", 2): n7, ("g", 0): n12}
    pv = {k: port.import_words(pc.words_of(pc.operand_bits(*k, nbits=nb)), True, nb) for k, nb in keys.items()}
    gv = pc.device_operands(bm, ctx, pv)
    groups = [([("a", 6), ("a", 7)], [("s", 1)]), ([("a", 6)], [("s", 2), ("s", 1)]), ([("a", 8), ("a", 6)], []),
              ([("g", 0), ("a", 7)], [("s", 1)]), ([("a", 6), ("g", 0)], [("a", 8)])]
    exp = pc.expected_csr(port, pv, groups, ncols=12)
    assert (np.diff(exp[0].astype(np.int64)) > 0).all() and exp[1].max() >= 11 * B
    _same(bm.aggregator(ctx).combine_and_sub_indices(pc.make_pipeline(bm, ctx, gv, groups)), exp)


@pytest.mark.parametrize("rng", [(2, 5), (0, 1), (6, 7), (5, 5), (0, 0xFFFFFFFF)])
def test_column_ranges(ctx, port, grid, rng):
    exp = pc.expected_csr(port, grid["pv"], grid["groups"], rng[0], rng[1])
    got = bm.aggregator(ctx).combine_and_sub_indices(grid["pipe"], rng[0], rng[1])
    _same(got, exp)
    if rng == (5, 5):
        assert got[1].size == 0 and (got[0] == 0).all()
    elif rng[0]:
        assert got[1].min() >= rng[0] * B                    # positions stay absolute


def test_width(ctx, grid):
    o4, i4 = bm.aggregator(ctx).combine_and_sub_indices(grid["pipe"], width=4)
    assert i4.dtype == np.uint32
    _same((o4, i4), (grid["offsets"], grid["ids"]))
    # 65,537 block columns: 32-bit positions cannot address them; 64-bit ones reach beyond 2^32
    ids = np.array([5, 77, 65535 * B + 7, 65535 * B + 65535, 65536 * B, 65536 * B + 9], np.uint64)
    v = bm.bvector.from_indices(ctx, ids)
    assert v.info()["nblocks"] == 65537
    pipe = pc.make_pipeline(bm, ctx, {"v": v}, [(["v"], []), (["v", "v"], [])])
    rc, n, _, _ = _raw(ctx, pipe, 0, 0xFFFFFFFF, 4, 16)
    assert rc == RANGE
    off, got = bm.aggregator(ctx).combine_and_sub_indices(pipe)
    assert (off == [0, 6, 12]).all() and (got == np.concatenate([ids, ids])).all() and got[-1] >= 1 << 32
    off, got = bm.aggregator(ctx).combine_and_sub_indices(pipe, 65535, 65537)
    assert (off == [0, 4, 8]).all() and (got[:4] == ids[2:]).all()


def test_capacity_protocol(ctx, grid):
    total = int(grid["offsets"][-1])
    for width in (8, 4):
        for cap in (0, total - 1):
            rc, n, off, out = _raw(ctx, grid["pipe"], 0, 0xFFFFFFFF, width, cap)
            assert rc == RANGE and n == total and (off == grid["offsets"]).all()
            assert (out == out.dtype.type(0xAB)).all()
        rc, n, off, out = _raw(ctx, grid["pipe"], 0, 0xFFFFFFFF, width, total)
        assert rc == 0 and n == total and (off == grid["offsets"]).all() and (out.astype(np.uint64) == grid["ids"]).all()
        rc, n, off, out = _raw(ctx, grid["pipe"], 0, 0xFFFFFFFF, width, total + 3)
        assert rc == 0 and n == total and (out[:total].astype(np.uint64) == grid["ids"]).all() and (out[total:] == out.dtype.type(0xAB)).all()


def test_chunk_borders(ctx, port, grid):
    """70 groups x 7 columns: the one-chunk run, chunks of 12 groups (1 KiB of table: 85 items; the last chunk holds 10) and
    chunks of a single group each (0) give the identical CSR"""
    groups = pc.chunk_groups()
    assert len(groups) == 70
    pipe = pc.make_pipeline(bm, ctx, grid["gv"], groups)
    exp = pc.expected_csr(port, grid["pv"], groups)
    agg = bm.aggregator(ctx)
    try:
        one = agg.combine_and_sub_indices(pipe)
        _same(one, exp)
        for kb in (1, 0):
            ctx.set_tuning("hits_table_kb", kb)
            got = agg.combine_and_sub_indices(pipe)
            _same(got, one)
            _same(agg.combine_and_sub_indices(pipe, 2, 5, width=4), pc.expected_csr(port, grid["pv"], groups, 2, 5))
    finally:
        ctx.set_tuning("hits_table_kb", 512 * 1024)


def test_scanner_batch(ctx):
    """2,048 values over 12 planes x 5 blocks of rows, with NULL rows, value 0, repeated values and a value whose set bit has no
    plane: every segment equals np.flatnonzero(col == v) over the rows that are not NULL"""
    rng = np.random.default_rng(2048)
    n = 5 * B - 37
    col = rng.integers(0, 4096, n).astype(np.uint64) & ~np.uint64(1 << 7)       # plane 7 does not exist
    col[rng.random(n) < 0.05] = 0
    isnull = rng.random(n) < 0.1
    stored = np.where(isnull, np.uint64(0), col)
    def upload(bits):
        return bm.bit_import_u32(ctx, pc.words_of(np.concatenate([bits.astype(np.uint8), np.zeros((-n) % 32, np.uint8)])), True)
    planes = []
    for i in range(12):
        bits = ((stored >> np.uint64(i)) & np.uint64(1)) != 0
        planes.append(upload(bits) if bits.any() else None)
    assert planes[7] is None and all(p is not None for i, p in enumerate(planes) if i != 7)
    sc = bm.slice_scanner(ctx, planes, size=n, not_null=upload(~isnull))
    values = rng.integers(1, 4096, 2048).astype(np.uint64) & ~np.uint64(1 << 7)
    values[[0, 100, 2047]] = 0
    values[[5, 900]] = 1 << 7 | 3                                               # a set bit without a plane
    values[[7, 8, 1500]] = values[6]                                            # repeated
    values[values == 0] = 0
    order = np.argsort(np.where(isnull, np.uint64(1 << 20), col), kind="stable")
    key = np.where(isnull, np.uint64(1 << 20), col)[order]
    parts = [order[np.searchsorted(key, v, "left"):np.searchsorted(key, v, "right")].astype(np.uint64) for v in values]
    assert parts[5].size == 0 and parts[0].size > 0 and sum(p.size > 0 for p in parts) > 1900
    assert (parts[3] == np.flatnonzero((col == values[3]) & ~isnull)).all()
    exp_off = np.zeros(2049, np.uint64); exp_off[1:] = np.cumsum([p.size for p in parts], dtype=np.uint64)
    off, ids = sc.find_eq_indices(values)
    _same((off, ids), (exp_off, np.concatenate(parts)))
    one = sc.find_eq_indices(int(values[3]))                                    # the single-value form is what it was
    assert (one == parts[3]).all()
    off, ids = sc.find_eq_indices(values[1:6])                                  # no zero, one impossible value: spliced too
    assert (off == exp_off[1:7] - exp_off[1]).all() and (ids == np.concatenate(parts[1:6])).all()


def test_prepared_collection(port):
    """a GAP-only pipeline: the same CSR before and after bmx_collection_prepare, in one chunk and in many (the per-group totals
    of a chunked run come from the counts run, which the collection's member directory then serves)"""
    nbits = 9 * B - 1234
    keys = [("h", i) for i in range(16)]
    pv = pc.oracle_operands(port, keys, nbits)
    assert all(set(v.flatten()[0].tolist()) == {pc.GAP} for v in pv.values())
    rng = np.random.default_rng(3)
    groups = []
    for k in range(9):
        sel = rng.permutation(16)
        na, ns = 1 + k % 3, k % 4
        groups.append(([("h", int(i)) for i in sel[:na]], [("h", int(i)) for i in sel[na:na + ns]]))
    exp = pc.expected_csr(port, pv, groups, ncols=9)
    assert (np.diff(exp[0].astype(np.int64)) > 0).all()
    c = bm.context(0)
    c.set_tuning("coll_members", 1)                          # (through the member directory also where the tables would be picked)
    gv = pc.device_operands(bm, c, pv)
    agg = bm.aggregator(c)
    pipe = pc.make_pipeline(bm, c, gv, groups)
    _same(agg.combine_and_sub_indices(pipe), exp)
    c.collection_prepare([gv[k] for k in keys], bm.ROLE_AND)
    c.collection_prepare([gv[k] for k in keys], bm.ROLE_OR)
    pipe2 = pc.make_pipeline(bm, c, gv, groups)
    for kb in (512 * 1024, 1, 0):
        c.set_tuning("hits_table_kb", kb)
        _same(agg.combine_and_sub_indices(pipe), exp)
        _same(agg.combine_and_sub_indices(pipe2), exp)
        _same(agg.combine_and_sub_indices(pipe2, 3, 8), pc.expected_csr(port, pv, groups, 3, 8, ncols=9))
    assert "k_coll_members" in pipe2.describe(), pipe2.describe()
    del pipe, pipe2, gv
    c.close()


def test_device_form(ctx, grid):
    import torch
    total = int(grid["offsets"][-1])
    ng = grid["pipe"].size()
    for width, dt in ((8, torch.int64), (4, torch.int32)):
        d_out = torch.full((total + 5,), -1, dtype=dt, device="cuda")
        d_off = torch.full((ng + 1,), -1, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        agg = bm.aggregator(ctx)
        off, n = agg.combine_and_sub_indices_dev(grid["pipe"], d_out.data_ptr(), total + 5, width=width, d_offsets_ptr=d_off.data_ptr())
        ctx.synchronize()
        assert n == total and (off == grid["offsets"]).all()
        assert (d_off.cpu().numpy().view(np.uint64) == grid["offsets"]).all()
        got = d_out.cpu().numpy()
        assert (got[:total].view(np.uint32 if width == 4 else np.uint64).astype(np.uint64) == grid["ids"]).all() and (got[total:] == -1).all()
        # too small: nothing written, the error carries the total and the offsets; no host offsets, no device offsets: both optional
        d_out.fill_(-1); torch.cuda.synchronize()
        with pytest.raises(bm.BmxError) as e:
            agg.combine_and_sub_indices_dev(grid["pipe"], d_out.data_ptr(), total - 1, width=width)
        ctx.synchronize()
        assert e.value.status == RANGE and e.value.n == total and (e.value.offsets == grid["offsets"]).all() and bool((d_out == -1).all())
        n2 = C.c_uint64()
        assert bm.lib().bmx_pipeline_run_indices_dev(ctx._h, grid["pipe"]._h, 0, 0xFFFFFFFF, width, None, None, C.c_void_p(d_out.data_ptr()),
                                                     total, C.byref(n2)) == 0
        ctx.synchronize()
        assert n2.value == total and (d_out.cpu().numpy()[:total].view(np.uint32 if width == 4 else np.uint64).astype(np.uint64) == grid["ids"]).all()


_REDZONE_SCRIPT = r'''
import ctypes as C, json, os, sys
sys.path.insert(0, os.getcwd())
sys.path.insert(0, os.path.join(os.getcwd(), "tests", "golden"))
import numpy as np
import bitmagic_amd as bm
import oracle
import pipe_indices_cases as pc
P = oracle.port()
ctx = bm.context(0)
out = {"enabled": ctx.redzone_check()["enabled"]}
pv = pc.oracle_operands(P)
gv = pc.device_operands(bm, ctx, pv)
agg = bm.aggregator(ctx)
def same(got, exp):
    return bool(got[0].shape == exp[0].shape and (got[0] == exp[0]).all() and got[1].shape == exp[1].shape and (got[1].astype(np.uint64) == exp[1]).all())
groups = pc.grid_groups()
pipe = pc.make_pipeline(bm, ctx, gv, groups)
exp = pc.expected_csr(P, pv, groups)
out["grid"] = same(agg.combine_and_sub_indices(pipe), exp) and same(agg.combine_and_sub_indices(pipe, width=4), exp)
total = int(exp[0][-1])
ok = True
for width in (8, 4):
    for cap in (0, total - 1, total):
        offs = np.zeros(len(groups) + 1, np.uint64)
        buf = np.full(max(cap, 1), 0xAB, np.uint64 if width == 8 else np.uint32)
        n = C.c_uint64()
        rc = bm.lib().bmx_pipeline_run_indices(ctx._h, pipe._h, 0, 0xFFFFFFFF, width, offs.ctypes.data_as(C.POINTER(C.c_uint64)), bm._ptr(buf), cap, C.byref(n))
        ok = ok and rc == (0 if cap == total else 3) and n.value == total and bool((offs == exp[0]).all())
        ok = ok and bool((buf.astype(np.uint64) == exp[1]).all() if cap == total else (buf == 0xAB).all())
out["capacity"] = ok
groups = pc.chunk_groups()
pipe = pc.make_pipeline(bm, ctx, gv, groups)
exp = pc.expected_csr(P, pv, groups)
ok = same(agg.combine_and_sub_indices(pipe), exp)
for kb in (1, 0):
    ctx.set_tuning("hits_table_kb", kb)
    ok = ok and same(agg.combine_and_sub_indices(pipe), exp) and same(agg.combine_and_sub_indices(pipe, 1, 6, 4), pc.expected_csr(P, pv, groups, 1, 6))
out["chunks"] = ok
del pipe
ctx.synchronize()
out["hits"] = ctx.redzone_check()["hits"]
print("REDZONE " + json.dumps(out))
'''


def test_red_zones_clean():
    """a fresh process under BMX_DEBUG_REDZONE=1: the kinds grid, the capacity protocol and the chunked run write nothing outside
    their allocations"""
    env = dict(os.environ, BMX_DEBUG_REDZONE="1")
    r = subprocess.run([sys.executable, "-c", _REDZONE_SCRIPT], capture_output=True, text=True, timeout=600, cwd=ROOT, env=env)
    line = [l for l in r.stdout.splitlines() if l.startswith("REDZONE ")]
    assert r.returncode == 0 and line, (r.stdout + r.stderr)[-3000:]
    out = json.loads(line[0][8:])
    assert out["enabled"] and out["hits"] == 0, out
    assert out["grid"] and out["capacity"] and out["chunks"], out


def test_no_leak(ctx, grid):
    """bmx_ctx_mem_used is back where it was after every kind of exit: success, BMX_ERR_RANGE for the capacity and for the width,
    one chunk and many, host and device form"""
    import torch
    total = int(grid["offsets"][-1])
    d_out = torch.zeros((total,), dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    agg = bm.aggregator(ctx)
    agg.combine_and_sub_indices(grid["pipe"])
    ctx.synchronize()
    base = ctx.mem_used()
    try:
        for kb in (512 * 1024, 1, 0):
            ctx.set_tuning("hits_table_kb", kb)
            _same(agg.combine_and_sub_indices(grid["pipe"]), (grid["offsets"], grid["ids"]))
            assert ctx.mem_used() == base
            for cap in (0, total - 1):
                assert _raw(ctx, grid["pipe"], 0, 0xFFFFFFFF, 8, cap)[0] == RANGE
                assert ctx.mem_used() == base
            assert _raw(ctx, grid["pipe"], 3, 2, 8, 4)[0] == RANGE              # nb_from > nb_to
            agg.combine_and_sub_indices_dev(grid["pipe"], d_out.data_ptr(), total)
            with pytest.raises(bm.BmxError):
                agg.combine_and_sub_indices_dev(grid["pipe"], d_out.data_ptr(), 1)
            ctx.synchronize()
            assert ctx.mem_used() == base
    finally:
        ctx.set_tuning("hits_table_kb", 512 * 1024)
