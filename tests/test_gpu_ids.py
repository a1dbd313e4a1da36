"""GPU: vectors built from id lists (bmx_vec_from_indices[_dev|_shard], bmx_gvec_from_indices, set / keep / clear; the kernels of
bmx_kernels13.h and k_scan_layout) against the constructed cases of tests/golden/ids_cases.py: size(), count() and the full block
table -- kinds, offsets, bit slab, GAP slab -- byte for byte against the closed form, for host and device ids, both widths and
every sort_order (the device decides the order: a false BM_SORTED is part of the test).  tests/test_ids_host.py proves that every
case meets the border its name claims and that the closed form is the oracle's and the reference's answer."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import bitmagic_amd as bm  # noqa: E402
from bitmagic_amd import _ffi  # noqa: E402

import ids_cases as ic  # noqa: E402

B = ic.B
ORDERS = (bm.BM_UNKNOWN, bm.BM_SORTED, bm.BM_UNSORTED, bm.BM_SORTED_UNIFORM)
CHUNK_IDS, CHUNK_CASES = 150_000, 24


def _chunks():
    """the cases in name order, cut into items of at most CHUNK_CASES cases and CHUNK_IDS ids (a larger case is an item of its own)"""
    out, cur, ids = [], [], 0
    for name in sorted(ic.CASES):
        c = ic.CASES[name]
        if cur and (cur[0].grid != c.grid or len(cur) == CHUNK_CASES or ids + c.n > CHUNK_IDS):
            out.append(cur); cur, ids = [], 0
        cur.append(c); ids += c.n
    out.append(cur)
    return out


CHUNKS = _chunks()


def _chunk_id(k):
    cs = CHUNKS[k]
    return cs[0].name if len(cs) == 1 else "%s..%s(%d)" % (cs[0].name, cs[-1].name.split("/", 1)[1], len(cs))


def _host(ids, width):
    return np.ascontiguousarray(ids, np.uint32 if width == 4 else np.uint64)


def _dev(ids, width):
    """the ids as a contiguous torch tensor on the GPU (32-bit ids arrive as int32), ready for another stream"""
    import torch
    a = _host(ids, width).view(np.int32 if width == 4 else np.int64)
    t = torch.from_numpy(a).cuda()
    torch.cuda.synchronize()
    return t


def _check(v, e, note):
    """size and the block table of v against the closed form e = (nbits, kinds, offs, bit_slab, gap_slab), level bits masked"""
    kinds, offs, bits, gaps = v.block_table()
    assert v.size() == e[0], note
    assert kinds.shape == e[1].shape and (kinds == e[1]).all(), note
    assert (offs == e[2]).all(), note
    assert bits.shape == e[3].shape and (bits == e[3]).all(), note
    assert gaps.shape == e[4].shape and (ic.mask_levels(kinds, offs, gaps) == ic.mask_levels(e[1], e[2], e[4])).all(), note


def _run(ctx, c, opt):
    ids = c.ids()
    e = c.expected(opt)
    uniq = c.uniq()
    large = c.n > ic.LARGE
    for width in c.widths()[:1] if large else c.widths():
        args = [("host", _host(ids, width)), ("dev", _dev(ids, width))]
        if width == 4 and c.grid == "I6": args.append(("host_int32", _host(ids, 4).view(np.int32)))
        for so in ORDERS[:1] if large else ORDERS:
            for src, arg in args:
                note = (c.name, opt, width, so, src)
                v = bm.bvector.from_indices(ctx, arg, c.nbits, so, bool(opt))
                _check(v, e, note)
                assert v.count() == uniq.size, note
                if e[1].size <= 64: assert (v.to_indices(8) == uniq).all(), note


@pytest.mark.parametrize("opt", [0, 1])
@pytest.mark.parametrize("k", range(len(CHUNKS)), ids=_chunk_id)
def test_tables_equal_the_closed_form(ctx, k, opt):
    for c in CHUNKS[k]:
        _run(ctx, c, opt)


def _shard(ctx, ids, width, so, nbits, f, t, opt):
    a = _host(ids, width)
    h = C.c_void_p()
    rc = bm.lib().bmx_vec_from_indices_shard(ctx._h, bm._ptr(a), width, a.size, so, nbits, f, t, opt, C.byref(h))
    return rc, (bm.bvector(ctx, h) if rc == 0 else None)


@pytest.mark.parametrize("name", [c.name for c in ic.grid("I5")])
def test_windows_of_the_nine_block_case(ctx, name):
    """every window [f, t) of 0 .. 9, t past the vector (clamped) and t = 0xFFFFFFFF: kinds, slabs and nbits of the shard are the
    windowed closed form; nb_from == nb_to gives zero blocks; nb_from beyond the clamped nb_to gives BMX_ERR_RANGE"""
    c = ic.CASES[name]
    ids = c.ids()
    for j, (f, t) in enumerate(ic.i5_windows()):
        for opt in (0, 1):
            rc, v = _shard(ctx, ids, 8 if (j + opt) & 1 else 4, ORDERS[j % 4], c.nbits, f, t, opt)
            assert rc == 0, (name, f, t)
            e = c.expected(opt, (f, t))
            _check(v, e, (name, f, t, opt))
            inside = c.uniq()[(c.uniq() >> np.uint64(16) >= f) & (c.uniq() >> np.uint64(16) < t)]
            assert v.count() == inside.size and v.info()["nblocks"] == min(t, 9) - f
            if f == t: assert v.info()["nblocks"] == 0 and v.size() == 0
    for f, t in ((10, 12), (10, ic.ALL), (5, 4), (1, 0)):
        rc, v = _shard(ctx, ids, 8, bm.BM_UNKNOWN, c.nbits, f, t, 1)
        assert rc == _ffi.ERR_RANGE and v is None, (f, t)
    rc, v = _shard(ctx, ids, 8, bm.BM_UNKNOWN, c.nbits, 9, 12, 1)                     # an empty window at the end of the vector
    assert rc == 0 and v.info()["nblocks"] == 0


@pytest.mark.parametrize("opt", [0, 1])
def test_windows_around_the_lds_border(ctx, opt):
    """the 16,385-block list: [0, 16384) takes the LDS form, [1, 16385) too, the whole vector does not"""
    c = ic.CASES["I2/lds_16385"]
    ids = c.ids()
    for w in ic.I5_LDS_WINDOWS:
        p = ic.plan(ids, c.nbits, w)
        assert p["lds"] == (w != (0, 16385)) and not p["sorted"]
        for width in (4, 8):
            rc, v = _shard(ctx, ids, width, bm.BM_UNKNOWN, c.nbits, w[0], w[1], opt)
            assert rc == 0
            _check(v, c.expected(opt, w), (w, opt, width))


@pytest.mark.parametrize("members", [2, 5])
def test_group_form_equals_the_single_table(ctx, members):
    grp = bm.group([0] * members)
    for name in ("I4/u/touched_513", "I4/s/touched_65", "I5/s/mixed9", "I5/u/mixed9"):
        c = ic.CASES[name]
        ids = c.ids()
        for opt in (0, 1):
            e = c.expected(opt)
            gv = bm.gbvector.from_indices(grp, ids, c.nbits, bm.BM_UNKNOWN, bool(opt))
            kinds, offs, bits, gaps = gv.block_table()
            assert gv.info()["nbits"] == e[0] and (kinds == e[1]).all() and gv.count() == c.uniq().size, (name, opt)
            assert ic.record(kinds, offs, bits, gaps) == ic.record(*e[1:]), (name, opt, members)
    grp.close()


def test_limits_come_back_as_status_and_leave_the_context_usable(ctx):
    """an id of 2^36 and nbits of 2^36 + 1 give BMX_ERR_RANGE (arguments only: nothing faults); the next call works and the
    context holds what it held"""
    c = ic.CASES["I6/w8_high"]
    ctx.synchronize(); ctx.trim()
    base = ctx.mem_used()
    for ids, nbits in ((np.array([5, 1 << 36], np.uint64), 0), (np.array([1 << 36, 5], np.uint64), 0), (np.array([5], np.uint64), (1 << 36) + 1)):
        for arg in (ids, _dev(ids, 8)):
            with pytest.raises(bm.BmxError) as ei:
                bm.bvector.from_indices(ctx, arg, nbits, bm.BM_UNKNOWN, True)
            assert ei.value.status == _ffi.ERR_RANGE
            rc, v = _shard(ctx, ids, 8, bm.BM_UNKNOWN, nbits, 0, 4, 1)
            assert rc == _ffi.ERR_RANGE
        v = bm.bvector.from_indices(ctx, c.ids(), 1 << 36, bm.BM_UNKNOWN, True)            # the largest vector there is
        _check(v, c.expected(True), "after an error")
        del v
    ctx.synchronize(); ctx.trim()
    assert ctx.mem_used() == base


_I3 = sorted(c.name for c in ic.grid("I3"))


@pytest.mark.parametrize("k", range(4))
def test_set_keep_clear_of_the_block_content_lists(ctx, k):
    """set / keep / clear of every I3 list on one base vector of three blocks: words and size() by NumPy set algebra"""
    nbits = 3 * B
    base = np.zeros(nbits, bool)
    base[np.arange(7, 3 * B, 3)] = True
    base[B + 100:B + 9000] = True
    base[[0, B - 1, B, 2 * B - 1, 2 * B, 3 * B - 1]] = True
    base_ids = np.flatnonzero(base).astype(np.uint64)
    for j, name in enumerate(_I3[k::4]):
        c = ic.CASES[name]
        ids = c.ids()
        lst = np.zeros(nbits, bool); lst[c.uniq().astype(np.int64)] = True
        for meth, exp in (("set", base | lst), ("keep", base & lst), ("clear", base & ~lst)):
            v = bm.bvector.from_indices(ctx, base_ids, nbits)
            width = 4 if (j + len(meth)) & 1 else 8
            getattr(v, meth)(_host(ids, width) if j % 3 else _dev(ids, width), ORDERS[j % 4])
            assert v.size() == nbits, (name, meth)
            assert (v.to_words(nbits // 32) == ic.words_of(exp)).all(), (name, meth, width)
            assert v.count() == int(exp.sum()), (name, meth)
