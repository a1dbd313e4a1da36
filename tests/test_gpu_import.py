"""GPU: vectors built from lists of bit positions (bvector::set(ids, n, sort_order) on an empty vector, src/bm.h:4153;
bmx_vec_from_indices[_dev|_shard], bmx_gvec_from_indices) against the reference fixture import_ref.json and the oracle port:
block tables byte for byte, for every order of the ids, and set / keep / clear against bmx_op2 of the oracle."""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import bitmagic_amd as bm  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, GOLDEN)
from import_cases import canonical, cases, oracle_table, record  # noqa: E402

with open(os.path.join(GOLDEN, "import_ref.json")) as _f:
    FIXTURE = json.load(_f)["cases"]
CASES = cases()
ORDERS = (bm.BM_UNSORTED, bm.BM_SORTED, bm.BM_SORTED_UNIFORM, bm.BM_UNKNOWN)


def _dev(ids, width):
    """the ids as a contiguous torch tensor on the GPU (32-bit ids reinterpreted as int32), ready for another stream"""
    import torch
    a = np.ascontiguousarray(ids, np.uint32).view(np.int32) if width == 4 else np.ascontiguousarray(ids, np.uint64).view(np.int64)
    t = torch.from_numpy(a.copy()).cuda()
    torch.cuda.synchronize()
    return t


def _host(ids, width):
    return np.ascontiguousarray(ids, np.uint32 if width == 4 else np.uint64)


def _widths(ids):
    return (4, 8) if (ids.size == 0 or int(ids.max()) < (1 << 32)) else (8,)


def _check_table(v, c_opt, nbits_out):
    kinds, offs, bits, gaps = v.block_table()
    assert v.size() == nbits_out
    assert record(kinds, offs, bits, gaps) == c_opt
    # the device writes the canonical layout itself: GAP blocks from 16-byte boundaries, 0xFFFF padding
    k, o, b, g = canonical(kinds, offs, bits, gaps)
    assert (o == offs).all()
    gm = gaps.copy()
    for nb in np.nonzero(kinds == bm.GAP)[0]:
        gm[offs[nb]] &= 0xFFF9
    assert (gm == g).all()


@pytest.mark.parametrize("name", sorted(CASES))
def test_fixture_cases(ctx, port, name):
    ids, nbits, _ = CASES[name]
    c = FIXTURE[name]
    uniq = np.unique(ids)
    for opt in (0, 1):
        _, ptable, pcount = oracle_table(port, ids, nbits, bool(opt))
        assert record(*ptable) == c[f"opt{opt}"]
        for width in _widths(ids):
            for src in ("host", "dev"):
                arg = _host(ids, width) if src == "host" else _dev(ids, width)
                v = bm.bvector.from_indices(ctx, arg, nbits, bm.BM_UNKNOWN, bool(opt))
                _check_table(v, c[f"opt{opt}"], c["nbits_out"])
                assert v.count() == c["count"] == pcount == uniq.size
                assert (v.to_indices(8) == uniq).all()


@pytest.mark.parametrize("name", ["mixed_blocks", "duplicates", "dense_beyond_2_32", "full_block"])
def test_order_and_flag_do_not_change_the_table(ctx, name):
    """the same ids in another order, under every sort_order -- a false BM_SORTED included -- give a byte-identical table"""
    ids, nbits, _ = CASES[name]
    rng = np.random.default_rng(7)
    for opt in (0, 1):
        ref = bm.bvector.from_indices(ctx, np.sort(ids), nbits, bm.BM_SORTED, bool(opt)).block_table()
        for trial in range(2):
            shuffled = rng.permutation(ids)
            for so in ORDERS:
                for width in _widths(ids):
                    for src in ("host", "dev"):
                        arg = _host(shuffled, width) if src == "host" else _dev(shuffled, width)
                        got = bm.bvector.from_indices(ctx, arg, nbits, so, bool(opt)).block_table()
                        for a, b in zip(got, ref):
                            assert a.dtype == b.dtype and a.shape == b.shape and (a == b).all(), (name, opt, so, width, src)


@pytest.mark.parametrize("dq", [6554, 655, 66])
def test_round_trip_through_device_indices(ctx, dq):
    """from_indices_dev(to_indices_dev(v), v.size(), BM_SORTED, optimize=1) == v for a generated vector (optimize=1: the same
    storage rule), representation and content, with no host copy of the ids"""
    import torch
    nbits = 2100 * 65536 + 321
    v = bm.bvector.generate(ctx, 0x1D5, 3, dq, nbits, optimize=True)
    cnt = v.count()
    for width, dt in ((4, torch.int32), (8, torch.int64)):
        d = torch.empty(cnt, dtype=dt, device="cuda")
        torch.cuda.synchronize()
        n = C.c_uint64()
        bm.check(bm.lib().bmx_vec_to_indices_dev(ctx._h, v._h, width, C.c_void_p(d.data_ptr()), cnt, C.byref(n)))
        assert n.value == cnt
        w = bm.bvector.from_indices(ctx, d, v.size(), bm.BM_SORTED, True)
        assert w.size() == v.size() and w.count() == cnt
        for a, b in zip(w.block_table(), v.block_table()):
            assert a.shape == b.shape and (a == b).all(), (dq, width)
        assert w.info()["counts"] == v.info()["counts"]


def test_sparse_ids_over_2_36_bits(ctx, port):
    """1e5 random ids over 2^36 bits (width 8): the vector has 2^20 blocks, ~1e5 of them touched"""
    rng = np.random.default_rng(36)
    ids = rng.integers(0, 1 << 36, size=100_000, dtype=np.uint64)
    ids[-1] = (1 << 36) - 1
    uniq = np.unique(ids)
    for opt in (0, 1):
        nbits_out, ptable, _ = oracle_table(port, ids, 0, bool(opt))
        for arg in (ids, _dev(ids, 8)):
            v = bm.bvector.from_indices(ctx, arg, 0, bm.BM_UNKNOWN, bool(opt))
            assert v.size() == 1 << 36 and v.info()["nblocks"] == 1 << 20
            assert record(*v.block_table()) == record(*ptable)
            assert v.count() == uniq.size and (v.to_indices(8) == uniq).all()


def test_set_keep_clear_follow_op2_of_the_oracle(ctx, port):
    nbits = 40 * 65536 + 11
    rng = np.random.default_rng(99)
    base_ids = np.unique(np.concatenate([rng.integers(0, nbits, 30000), 5 * 65536 + np.arange(65536)])).astype(np.uint64)
    lists = {"random": rng.integers(0, nbits, 5000).astype(np.uint64),
             "overlap": base_ids[::7].copy(),
             "empty": np.zeros(0, np.uint64),
             "longer": np.concatenate([rng.integers(0, nbits, 100), [nbits + 3 * 65536 + 9]]).astype(np.uint64),
             "dense": 9 * 65536 + np.arange(0, 65536, 2, dtype=np.uint64)}
    pv = port.new(nbits)
    for p in base_ids:
        pv.set_bit(int(p))
    for lname, ids in lists.items():
        for meth, op in (("set", bm.OR), ("keep", bm.AND), ("clear", bm.SUB)):
            for width in _widths(ids):
                v = bm.bvector.from_indices(ctx, base_ids, nbits)
                getattr(v, meth)(_host(ids, width))
                if ids.size == 0:
                    exp = port.new(nbits) if op == bm.AND else pv           # keep(): cleared; set() / clear(): unchanged
                    exp_nbits = nbits
                else:
                    exp_nbits = max(nbits, int(ids.max()) + 1)
                    pi = port.new(exp_nbits)
                    for p in ids: pi.set_bit(int(p))
                    exp = port.op2(op, pv, pi)
                assert v.size() == exp_nbits, (lname, meth)
                nw = ((exp_nbits + 65535) // 65536) * 2048
                assert (v.to_words(nw) == exp.to_words(nw)).all(), (lname, meth, width)
                assert v.count() == exp.count()


@pytest.mark.parametrize("members", [1, 3, 8])
def test_group_form_equals_single_gpu_table(ctx, members):
    grp = bm.group([0] * members)
    for name in ("mixed_blocks", "trailing_null_blocks", "ids_beyond_2_32", "empty_explicit_nbits"):
        ids, nbits, _ = CASES[name]
        for opt in (0, 1):
            for so in (bm.BM_SORTED, bm.BM_UNSORTED):
                arg = np.sort(ids) if so == bm.BM_SORTED else np.random.default_rng(1).permutation(ids)
                gv = bm.gbvector.from_indices(grp, arg, nbits, so, bool(opt))
                assert gv.info()["nbits"] == FIXTURE[name]["nbits_out"]
                assert record(*gv.block_table()) == FIXTURE[name][f"opt{opt}"], (name, opt, members)
                assert gv.count() == FIXTURE[name]["count"]
    grp.close()


def test_allocation_failures_come_back_as_status(ctx):
    """kinds 4 and 6 of bmx_debug_inject_failure over the new entries: BMX_ERR_BADALLOC, nothing leaks, the next call works"""
    c = bm.context(0)
    ids, nbits, _ = CASES["mixed_blocks"]
    exp = record(*bm.bvector.from_indices(c, ids, nbits, bm.BM_SORTED, True).block_table())
    shuffled = np.random.default_rng(3).permutation(ids)
    shard = (2, 8)
    def sorted_host(): return record(*bm.bvector.from_indices(c, ids, nbits, bm.BM_SORTED, True).block_table()) == exp
    def unsorted_host(): return record(*bm.bvector.from_indices(c, shuffled, nbits, bm.BM_UNKNOWN, True).block_table()) == exp
    d = _dev(shuffled, 4)
    def unsorted_dev(): return record(*bm.bvector.from_indices(c, d, nbits, bm.BM_UNKNOWN, True).block_table()) == exp
    def shard_host():
        h = C.c_void_p()
        a = _host(shuffled, 8)
        bm.check(bm.lib().bmx_vec_from_indices_shard(c._h, bm._ptr(a), 8, a.size, bm.BM_UNKNOWN, nbits, shard[0], shard[1], 1, C.byref(h)))
        v = bm.bvector(c, h)
        inside = ids[((ids >> 16) >= shard[0]) & ((ids >> 16) < shard[1])]
        return v.info()["nblocks"] == shard[1] - shard[0] and v.count() == np.unique(inside).size
    def set_op():
        v = bm.bvector.from_indices(c, ids[:100], nbits)
        v.set(shuffled)
        return v.count() == np.unique(ids).size
    for name, fn in (("sorted_host", sorted_host), ("unsorted_host", unsorted_host), ("unsorted_dev", unsorted_dev),
                     ("shard_host", shard_host), ("set", set_op)):
        assert fn(), name
        c.synchronize(); c.trim()
        base = c.mem_used()
        for kind in (4, 6):
            failed = 0
            for k in range(0, 24):
                c.inject_failure(kind, k)
                try:
                    assert fn(), (name, kind, k)
                except bm.BmxError as e:
                    assert e.status == 1, (name, kind, k, str(e))
                    failed += 1
                finally:
                    c.inject_failure(0, 0)
                c.synchronize()
            assert fn(), (name, kind)
            c.synchronize()
            assert failed >= 1, (name, kind)
        c.trim()
        leaked = c.mem_used() - base
        assert leaked <= (2 << 20), (name, leaked)
    c.close()
