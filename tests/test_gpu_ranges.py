"""GPU: vectors built from lists of inclusive [left, right] pairs (bvector::set_range per pair on an empty vector, then
optimize(), src/bm.h:2398; bmx_vec_from_ranges[_dev|_shard], bmx_gvec_from_ranges) and vectors returned as their intervals
(bm::interval_enumerator, src/bmintervals.h:52-226; bmx_vec_to_ranges[_dev]) against the reference fixture range_ref.json and the
oracle port: block tables byte for byte for every order of the pairs, intervals pair for pair, and set_range / clear_range /
keep_range against op2 of the oracle."""
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
GOLDEN = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, GOLDEN)
from import_cases import canonical  # noqa: E402
from range_cases import cases, oracle_table, orders, record, runs_of_words, sha  # noqa: E402

with open(os.path.join(GOLDEN, "range_ref.json")) as _f:
    FIXTURE = json.load(_f)["cases"]
CASES = cases()
B = 65536


def _dev(pairs, width):
    """the pairs as a contiguous (n, 2) torch tensor on the GPU (unsigned reinterpreted as signed), ready for another stream"""
    import torch
    a = np.ascontiguousarray(pairs, np.uint32).view(np.int32) if width == 4 else np.ascontiguousarray(pairs, np.uint64).view(np.int64)
    t = torch.from_numpy(a.copy().reshape(-1, 2)).cuda()
    torch.cuda.synchronize()
    return t


def _host(pairs, width):
    return np.ascontiguousarray(pairs, np.uint32 if width == 4 else np.uint64).reshape(-1, 2)


def _widths(pairs):
    return (4, 8) if (pairs.size == 0 or int(pairs.max()) < (1 << 32)) else (8,)


def _check_table(v, rec, nbits_out):
    kinds, offs, bits, gaps = v.block_table()
    assert v.size() == nbits_out
    assert record(kinds, offs, bits, gaps) == rec
    # the device writes the canonical layout itself: GAP blocks from 16-byte boundaries, 0xFFFF padding
    k, o, b, g = canonical(kinds, offs, bits, gaps)
    assert (o == offs).all()
    gm = gaps.copy()
    for nb in np.nonzero(kinds == bm.GAP)[0]:
        gm[offs[nb]] &= 0xFFF9
    assert (gm == g).all()
    return kinds, offs, bits, gaps


def _to_ranges_dev(ctx, v, width, cap=None):
    import torch
    n = C.c_uint64()
    rc = bm.lib().bmx_vec_to_ranges_dev(ctx._h, v._h, width, None, 0, C.byref(n))
    if rc not in (0, 3):
        bm.check(rc)
    cap = n.value if cap is None else cap
    d = torch.zeros((max(cap, 1), 2), dtype=torch.int32 if width == 4 else torch.int64, device="cuda")
    torch.cuda.synchronize()
    got = v.to_ranges_dev(d[:cap])
    torch.cuda.synchronize()
    return d[:got], got


def _expected(port, name):
    pairs, nbits, _ = CASES[name]
    c = FIXTURE[name]
    nbits_out, ptable, pcount, runs = oracle_table(port, pairs, nbits)
    assert record(*ptable) == c["table"] and pcount == c["count"] and nbits_out == c["nbits_out"]
    assert runs.shape[0] == c["intervals"] and sha(runs.astype("<u8")) == c["intervals_sha"]
    return runs


@pytest.mark.parametrize("name", sorted(CASES))
def test_fixture_cases(ctx, port, name):
    """every fixture case: the table of the reference in the device's layout, size, count, intervals -- for both widths, host and
    device input, and every order of the pairs (byte-identical tables)"""
    pairs, nbits, _ = CASES[name]
    c = FIXTURE[name]
    runs = _expected(port, name)
    first = None
    for oname, p in orders(pairs).items():
        for width in _widths(pairs):
            for src in ("host", "dev"):
                arg = _host(p, width) if src == "host" else _dev(p, width)
                v = bm.bvector.from_ranges(ctx, arg, nbits)
                table = _check_table(v, c["table"], c["nbits_out"])
                assert v.count() == c["count"], (name, oname, width, src)
                assert v.info()["counts"] == c["table"]["counts"]
                if first is None:
                    first = table
                for a, b in zip(table, first):
                    assert a.dtype == b.dtype and a.shape == b.shape and (a == b).all(), (name, oname, width, src)
                if oname in ("given", "shuffled1"):
                    got = v.to_ranges(width)
                    assert got.dtype == (np.uint32 if width == 4 else np.uint64) and got.shape == runs.shape
                    assert (got.astype(np.uint64) == runs).all(), (name, oname, width, src)
                    d, n = _to_ranges_dev(ctx, v, width)
                    assert n == runs.shape[0]
                    dn = d.cpu().numpy().view(np.uint32 if width == 4 else np.uint64).astype(np.uint64)
                    assert dn.shape == runs.shape and (dn == runs).all(), (name, oname, width, src)


def test_to_ranges_buffer_rule(ctx):
    """cap too small: BMX_ERR_RANGE, *n = the number needed, the buffer untouched; an empty vector: 0 intervals"""
    pairs, nbits, _ = CASES["random_4000"]
    need = FIXTURE["random_4000"]["intervals"]
    v = bm.bvector.from_ranges(ctx, pairs, nbits)
    for width, dt in ((4, np.uint32), (8, np.uint64)):
        buf = np.full((need, 2), 0xAB, dt)
        n = C.c_uint64()
        assert bm.lib().bmx_vec_to_ranges(ctx._h, v._h, width, bm._ptr(buf), need - 1, C.byref(n)) == 3
        assert n.value == need and (buf == 0xAB).all()
        import torch
        d = torch.full((need, 2), 0x55, dtype=torch.int32 if width == 4 else torch.int64, device="cuda")
        torch.cuda.synchronize()
        n = C.c_uint64()
        assert bm.lib().bmx_vec_to_ranges_dev(ctx._h, v._h, width, C.c_void_p(d.data_ptr()), 1, C.byref(n)) == 3
        ctx.synchronize()
        assert n.value == need and bool((d == 0x55).all())
        assert bm.lib().bmx_vec_to_ranges(ctx._h, v._h, width, bm._ptr(buf), need, C.byref(n)) == 0 and n.value == need
    for e in (bm.bvector.from_ranges(ctx, np.zeros((0, 2), np.uint64), 3 * B + 7), bm.bvector.from_ranges(ctx, [], 0),
              bm.bvector.generate(ctx, 1, 1, 0, 5 * B)):
        assert e.to_ranges().shape == (0, 2) and e.to_ranges(4).shape == (0, 2)
    # width 4 cannot address a vector beyond 2^32 bits
    big = bm.bvector.from_ranges(ctx, np.array([[5, (1 << 32) + 9]], np.uint64))
    n = C.c_uint64()
    assert bm.lib().bmx_vec_to_ranges(ctx._h, big._h, 4, None, 0, C.byref(n)) == 3
    assert (big.to_ranges(8) == np.array([[5, (1 << 32) + 9]], np.uint64)).all()


def _generated(ctx, port):
    """(name, device vector, the port's words) for bit-blocks, GAP blocks, a mix, unoptimised forms, op2 results, FULL stretches"""
    nbits = 37 * B + 321
    nw = ((nbits + B - 1) // B) * 2048
    seed = 0x4A11
    out = []
    words = {}
    for vid, dq, opt in ((1, 30000, True), (2, 6554, True), (3, 655, True), (4, 66, True), (5, 6554, False), (6, 66, False), (7, 2000, True)):
        v = bm.bvector.generate(ctx, seed, vid, dq, nbits, optimize=opt)
        words[vid] = port.import_words(port.gen_words(seed, vid, dq, nbits), opt, nbits).to_words(nw)
        out.append((f"gen{vid}_dq{dq}_opt{int(opt)}", v, words[vid]))
    gv = {n.split("_")[0]: v for n, v, _ in out}
    out.append(("or_1_3", bm.bvector.bit_or(gv["gen1"], gv["gen3"]), words[1] | words[3]))
    out.append(("and_2_7", bm.bvector.bit_and(gv["gen2"], gv["gen7"], bm.opt_compress), words[2] & words[7]))
    out.append(("sub_1_2", bm.bvector.bit_sub(gv["gen1"], gv["gen2"]), words[1] & ~words[2]))
    out.append(("xor_3_4", bm.bvector.bit_xor(gv["gen3"], gv["gen4"], bm.opt_compress), words[3] ^ words[4]))
    full = bm.bvector.from_ranges(ctx, np.array([[3 * B - 5, 9 * B + 2], [20 * B, 30 * B - 1], [36 * B, 37 * B + 320]], np.uint64), nbits)
    fb = np.zeros(nw * 32, np.uint8)
    for l, r in ((3 * B - 5, 9 * B + 2), (20 * B, 30 * B - 1), (36 * B, 37 * B + 320)):
        fb[l:r + 1] = 1
    fw = np.packbits(fb, bitorder="little").view(np.uint32)
    out.append(("full_or_gen3", bm.bvector.bit_or(full, gv["gen3"]), fw | words[3]))
    out.append(("full_xor_gen2", bm.bvector.bit_xor(full, gv["gen2"]), fw ^ words[2]))
    return nbits, out


def test_round_trip_on_generated_vectors(ctx, port):
    """to_ranges equals the runs of the oracle port's words; from_ranges(to_ranges_dev(v)) has the table of the optimised v and
    count_xor 0 with it"""
    nbits, vecs = _generated(ctx, port)
    nw = ((nbits + B - 1) // B) * 2048
    for name, v, w in vecs:
        w = np.ascontiguousarray(w, np.uint32)
        assert w.size == nw and (v.to_words(nw) == w).all(), name
        runs = runs_of_words(w)
        for width in (4, 8):
            got = v.to_ranges(width)
            assert got.shape == runs.shape and (got.astype(np.uint64) == runs).all(), (name, width)
            d, n = _to_ranges_dev(ctx, v, width)
            assert n == runs.shape[0], (name, width)
            back = bm.bvector.from_ranges(ctx, d, nbits)
            assert back.size() == v.size() and back.count() == v.count()
            assert bm.count_xor(back, v) == 0, (name, width)
            exp = port.import_words(w, True, nbits).flatten()
            assert record(*back.block_table()) == record(*exp), (name, width)
            # the intervals of a vector are sorted and separated: any other order of them gives the same table
            import torch
            shuffled = d[torch.from_numpy(np.random.default_rng(4).permutation(n)).cuda()].contiguous() if n else d
            torch.cuda.synchronize()
            again = bm.bvector.from_ranges(ctx, shuffled, nbits)
            for a, b in zip(again.block_table(), back.block_table()):
                assert a.shape == b.shape and (a == b).all(), (name, width)


def test_one_pair_over_2_35_bits(ctx):
    """nothing scales with the covered bits: 524,288 FULL blocks, no bit-block, GAP words of at most the two end blocks"""
    l, r = 7 * B + 100, 7 * B + 100 + (1 << 35) - 1
    for arg in (np.array([[l, r]], np.uint64), np.array([[r, l]], np.uint64), _dev(np.array([[l, r]], np.uint64), 8),
                np.array([[l, r], [l + 5, l + 9]], np.uint64)):
        ctx.synchronize(); ctx.trim()
        base = ctx.mem_used()
        v = bm.bvector.from_ranges(ctx, arg)
        i = v.info()
        assert i["nbits"] == r + 1 and i["nblocks"] == 7 + 524288 + 1
        assert i["counts"][bm.FULL] == 524287 and i["counts"][bm.GAP] == 2 and i["counts"][bm.BIT] == 0 and i["counts"][bm.NULL] == 7
        assert i["bit_slab_blocks"] == 0 and i["gap_words"] <= 16
        assert v.count() == 1 << 35
        assert (v.to_ranges(8) == np.array([[l, r]], np.uint64)).all()
        assert ctx.mem_used() - base < (64 << 20)              # descriptors and per-block scratch of 524,296 blocks, not 64 GiB of bits
    # exactly 524,288 FULL blocks when the pair is block-aligned
    v = bm.bvector.from_ranges(ctx, np.array([[B, B + (1 << 35) - 1]], np.uint64))
    i = v.info()
    assert i["counts"] == [1, 524288, 0, 0] and i["bit_slab_blocks"] == 0 and i["gap_words"] == 0
    assert (v.to_ranges(8) == np.array([[B, B + (1 << 35) - 1]], np.uint64)).all()


@pytest.mark.parametrize("name", ["overlap_nested_dup", "random_4000", "long_span", "every_7_bits"])
def test_shards_concatenate_to_the_single_table(ctx, name):
    pairs, nbits, _ = CASES[name]
    whole = bm.bvector.from_ranges(ctx, pairs, nbits)
    wk, wo, wb, wg = whole.block_table()
    nblocks = whole.info()["nblocks"]
    nbits_out = whole.size()
    for cuts in ((0, 1, nblocks), (0, nblocks // 2, nblocks), (0, 2, nblocks - 1, nblocks)):
        for order in ("given", "sorted"):
            p = orders(pairs)[order]
            kinds, bits, gaps, total_bits = [], [], [], 0
            for lo, hi in zip(cuts[:-1], cuts[1:]):
                h = C.c_void_p()
                a = _host(p, 8)
                bm.check(bm.lib().bmx_vec_from_ranges_shard(ctx._h, bm._ptr(a), 8, a.shape[0], nbits, lo, hi, C.byref(h)))
                s = bm.bvector(ctx, h)
                assert s.info()["nblocks"] == hi - lo
                k, o, b, g = s.block_table()
                kinds.append(k); total_bits += s.size()
                for nb in range(k.size):
                    if k[nb] == bm.BIT:
                        bits.append(b[o[nb] * 2048:(o[nb] + 1) * 2048])
                    elif k[nb] == bm.GAP:
                        n = ((int(g[o[nb]]) >> 3) + 1 + 7) & ~7
                        gaps.append(g[o[nb]:o[nb] + n])
            assert total_bits == nbits_out
            assert (np.concatenate(kinds) == wk).all(), (name, cuts, order)
            assert (np.concatenate(bits) if bits else np.zeros(0, np.uint32)).tobytes() == wb.tobytes(), (name, cuts, order)
            assert (np.concatenate(gaps) if gaps else np.zeros(0, np.uint16)).tobytes() == wg.tobytes(), (name, cuts, order)


@pytest.mark.parametrize("members", [1, 3, 8])
def test_group_form_equals_single_gpu_table(ctx, members):
    grp = bm.group([0] * members)
    for name in ("overlap_nested_dup", "random_4000", "long_span", "beyond_2_32", "empty", "every_7_bits"):
        pairs, nbits, _ = CASES[name]
        for order in ("given", "sorted"):
            gv = bm.gbvector.from_ranges(grp, orders(pairs)[order], nbits)
            assert gv.info()["nbits"] == FIXTURE[name]["nbits_out"]
            assert record(*gv.block_table()) == FIXTURE[name]["table"], (name, order, members)
            assert gv.count() == FIXTURE[name]["count"]
    grp.close()


def test_set_clear_keep_range_follow_op2_of_the_oracle(ctx, port):
    nbits = 40 * B + 11
    seed = 0x5E7
    OPS = (("set_range", bm.OR), ("clear_range", bm.SUB), ("keep_range", bm.AND))
    ranges = ((5, 5), (100, 3 * B + 7), (3 * B + 7, 100), (B, 2 * B - 1), (39 * B, nbits - 1), (0, nbits - 1),
              (10 * B + 5, nbits + 2 * B + 9), (nbits + 5, nbits + 9))
    for vid, dq, opt in ((1, 30000, True), (2, 655, True), (3, 6554, False)):
        w = port.gen_words(seed, vid, dq, nbits)
        pv = port.import_words(w, opt, nbits)
        for l, r in ranges:
            for meth, op in OPS:
                v = bm.bvector.generate(ctx, seed, vid, dq, nbits, optimize=opt)
                getattr(v, meth)(l, r)
                exp_nbits = max(nbits, max(l, r) + 1)
                pr = port.new(exp_nbits)
                pr.set_range(min(l, r), max(l, r))
                exp = port.op2(op, pv, pr)
                assert v.size() == exp_nbits, (vid, l, r, meth)
                nw = ((exp_nbits + B - 1) // B) * 2048
                assert (v.to_words(nw) == exp.to_words(nw)).all(), (vid, l, r, meth)
                assert v.count() == exp.count()
        v = bm.bvector.generate(ctx, seed, vid, dq, nbits, optimize=opt)
        v.set_range(7, 9 * B, False)                           # value = false clears
        u = bm.bvector.generate(ctx, seed, vid, dq, nbits, optimize=opt).clear_range(7, 9 * B)
        assert bm.count_xor(u, v) == 0 and v.count() == u.count()


_REDZONE_SCRIPT = r'''
import json, os, sys
sys.path.insert(0, os.getcwd())
sys.path.insert(0, os.path.join(os.getcwd(), "tests", "golden"))
import numpy as np
import bitmagic_amd as bm
from range_cases import cases, orders
ctx = bm.context(0)
out = {"enabled": ctx.redzone_check()["enabled"], "counts": {}}
C = cases()
for name in ("overlap_nested_dup", "random_4000", "every_7_bits", "runs_1275", "runs_1276", "ends_at_65535", "long_span", "empty"):
    pairs, nbits, _ = C[name]
    for oname in ("given", "sorted", "shuffled1"):
        for dt in (np.uint32, np.uint64):
            v = bm.bvector.from_ranges(ctx, np.ascontiguousarray(orders(pairs)[oname], dt), nbits)
            r = v.to_ranges(np.dtype(dt).itemsize)
            w = bm.bvector.from_ranges(ctx, r, nbits)
            assert bm.count_xor(v, w) == 0
            out["counts"][name] = v.count()
g = bm.bvector.generate(ctx, 9, 1, 6554, 20 * 65536 + 5)
g.set_range(100, 70000).clear_range(3 * 65536, 5 * 65536 - 1).keep_range(50, 19 * 65536)
out["kept"] = int(g.to_ranges().shape[0])
grp = bm.group([0, 0, 0])
gv = bm.gbvector.from_ranges(grp, C["random_4000"][0], 0)
out["group"] = gv.count()
del gv
grp.close()
ctx.synchronize()
out["hits"] = ctx.redzone_check()["hits"]
print("REDZONE " + json.dumps(out))
'''


def test_red_zones_clean():
    """a fresh process under BMX_DEBUG_REDZONE=1: both import paths, GAP / bit / FULL emit, to_ranges and the range methods write
    nothing outside their allocations"""
    env = dict(os.environ, BMX_DEBUG_REDZONE="1")
    r = subprocess.run([sys.executable, "-c", _REDZONE_SCRIPT], capture_output=True, text=True, timeout=600, cwd=ROOT, env=env)
    line = [l for l in r.stdout.splitlines() if l.startswith("REDZONE ")]
    assert r.returncode == 0 and line, (r.stdout + r.stderr)[-3000:]
    out = json.loads(line[0][8:])
    assert out["enabled"] and out["hits"] == 0, out
    for name, cnt in out["counts"].items():
        assert cnt == FIXTURE[name]["count"], name
    assert out["group"] == FIXTURE["random_4000"]["count"] and out["kept"] > 0


def test_allocation_failures_come_back_as_status():
    """bmx_debug_inject_failure kind 4 in each path: BMX_ERR_BADALLOC, bmx_ctx_mem_used back where it started, the next call works"""
    c = bm.context(0)
    pairs, nbits, _ = CASES["random_4000"]
    exp = FIXTURE["random_4000"]
    srt = orders(pairs)["sorted"]
    merged = bm.bvector.from_ranges(c, pairs, nbits).to_ranges(8)             # sorted and separated
    d = _dev(pairs, 8)
    def sorted_host(): return record(*bm.bvector.from_ranges(c, merged, nbits).block_table()) == exp["table"]
    def any_host(): return record(*bm.bvector.from_ranges(c, srt, nbits).block_table()) == exp["table"]
    def any_dev(): return record(*bm.bvector.from_ranges(c, d, nbits).block_table()) == exp["table"]
    def shard_host():
        h = C.c_void_p()
        bm.check(bm.lib().bmx_vec_from_ranges_shard(c._h, bm._ptr(pairs), 8, pairs.shape[0], nbits, 2, 8, C.byref(h)))
        return bm.bvector(c, h).info()["nblocks"] == 6
    v = bm.bvector.from_ranges(c, pairs, nbits)
    def to_host(): return v.to_ranges(8).shape[0] == exp["intervals"]
    def to_dev(): return _to_ranges_dev(c, v, 8)[1] == exp["intervals"]
    def set_op():
        u = bm.bvector.from_ranges(c, merged[:50], nbits)
        u.set_range(5, 9 * B)
        return u.count() > 9 * B - 5
    for name, fn in (("sorted_host", sorted_host), ("any_host", any_host), ("any_dev", any_dev), ("shard_host", shard_host),
                     ("to_host", to_host), ("to_dev", to_dev), ("set_range", set_op)):
        assert fn(), name
        c.synchronize(); c.trim()
        base = c.mem_used()
        failed = 0
        for k in range(0, 24):
            c.inject_failure(4, k)
            try:
                assert fn(), (name, k)
            except bm.BmxError as e:
                assert e.status == 1, (name, k, str(e))
                failed += 1
            finally:
                c.inject_failure(0, 0)
            c.synchronize()
        assert fn(), name
        c.synchronize()
        assert failed >= 1, name
        c.trim()
        leaked = c.mem_used() - base
        assert leaked <= (2 << 20), (name, leaked)
    del v
    c.close()
