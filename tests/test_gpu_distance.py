"""GPU: bm::distance_operation (src/bmalgo_impl.h:766) and all-pairs distance matrices (bmx_distance, bmx_distance_matrix,
bmx_distance_matrix_dev, bmx_gdistance_matrix) against the oracle port, bit-exact."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import bitmagic_amd as bm  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 0xD157
ALL = (bm.COUNT_AND, bm.COUNT_XOR, bm.COUNT_OR, bm.COUNT_SUB_AB, bm.COUNT_SUB_BA, bm.COUNT_A, bm.COUNT_B)


def _expect(P, x, y, m):
    """metric m of (x, y) from the oracle"""
    if m == bm.COUNT_AND: return P.count_op2(bm.AND, x, y)
    if m == bm.COUNT_XOR: return P.count_op2(bm.XOR, x, y)
    if m == bm.COUNT_OR: return P.count_op2(bm.OR, x, y)
    if m == bm.COUNT_SUB_AB: return P.count_op2(bm.SUB, x, y)
    if m == bm.COUNT_SUB_BA: return P.count_op2(bm.SUB, y, x)
    if m == bm.COUNT_A: return x.count()
    return y.count()


def _pair(ctx, P, vid, dq, nbits, common=False):
    d = bm.bvector.generate(ctx, SEED, vid, dq, nbits, with_common=common)
    o = P.import_words(P.gen_words(SEED, vid, dq, nbits, with_common=common), True, nbits)
    return d, o


def _null_full(ctx, P, vid, nbits):
    """a vector with explicit NULL and FULL blocks next to bit / GAP ones (bmx_vec_upload of an edited block table)"""
    d, _ = _pair(ctx, P, vid, 655, nbits)
    kinds, offs, bits, gaps = d.block_table()
    kinds = kinds.copy()
    kinds[0] = bm.FULL
    kinds[2] = bm.NULL
    if kinds.size > 4:
        kinds[4] = bm.FULL
    dv = bm.bvector.from_block_table(ctx, nbits, kinds, offs, bits, gaps)
    return dv, P.from_table(nbits, kinds, offs, bits, gaps)


def _operand_pairs(ctx, P):
    nb = 6 * 65536 - 333
    ab, ob = _pair(ctx, P, 1, 6554, nb, True)
    ab2, ob2 = _pair(ctx, P, 2, 6554, nb, True)
    am, om = _pair(ctx, P, 3, 655, nb)
    am2, om2 = _pair(ctx, P, 4, 655, nb)
    ag, og = _pair(ctx, P, 5, 66, nb)
    ag2, og2 = _pair(ctx, P, 6, 200, nb)
    an, on = _null_full(ctx, P, 7, nb)
    an2, on2 = _null_full(ctx, P, 8, nb)
    ashort, oshort = _pair(ctx, P, 9, 6554, 2 * 65536 + 5)
    return {
        "all_bit": ((ab, ob), (ab2, ob2)),
        "mixed_1pct": ((am, om), (am2, om2)),
        "all_gap": ((ag, og), (ag2, og2)),
        "null_full": ((an, on), (am, om)),
        "null_full_both": ((an, on), (an2, on2)),
        "lengths_ab": ((ab, ob), (ashort, oshort)),
        "lengths_ba": ((ashort, oshort), (am, om)),
        "self": ((am, om), (am, om)),
        "self_null_full": ((an, on), (an, on)),
    }


@pytest.fixture(scope="module")
def pairs(ctx, port):
    return _operand_pairs(ctx, port)


@pytest.mark.parametrize("case", ["all_bit", "mixed_1pct", "all_gap", "null_full", "null_full_both", "lengths_ab", "lengths_ba",
                                  "self", "self_null_full"])
def test_distance_operation_every_metric(ctx, port, pairs, case):
    (a, oa), (b, ob) = pairs[case]
    got = bm.distance_operation(a, b, ALL)
    assert got == [_expect(port, oa, ob, m) for m in ALL], case
    # one metric at a time and repeated metrics give the same values
    assert bm.distance_operation(a, b, [bm.COUNT_B, bm.COUNT_AND, bm.COUNT_B]) == [got[6], got[0], got[6]]


def test_distance_operation_long_all_bit_stream(ctx, port):
    """>= 2,048 bit-blocks on both sides, equal lengths: the streaming form"""
    nbits = 2100 * 65536
    a = bm.bvector.generate(ctx, SEED, 11, 32768, nbits)
    b = bm.bvector.generate(ctx, SEED, 12, 32768, nbits)
    assert a.calc_stat()["bit_blocks"] == 2100
    got = bm.distance_operation(a, b, ALL)
    ab, ca, cb = bm.count_and(a, b), a.count(), b.count()
    assert got == [ab, ca + cb - 2 * ab, ca + cb - ab, ca - ab, cb - ab, ca, cb]


def test_distance_operation_long_mixed_loop(ctx, port):
    """>= 2,048 blocks of mixed kinds: the persistent loop form, against the count_* calls (themselves oracle-checked)"""
    nbits = 2300 * 65536 + 99
    a = bm.bvector.generate(ctx, SEED, 13, 655, nbits)
    b = bm.bvector.generate(ctx, SEED, 14, 66, nbits - 70 * 65536)
    got = bm.distance_operation(a, b, ALL)
    ab, ca, cb = bm.count_and(a, b), a.count(), b.count()
    assert got == [ab, bm.count_xor(a, b), bm.count_or(a, b), bm.count_sub(a, b), bm.count_sub(b, a), ca, cb]


def _pool(ctx, P, n, base=100):
    """n small vectors of mixed kinds and lengths (1..4 blocks + a tail)"""
    dqs = (6554, 655, 66, 32768, 0, 200, 65536)
    out = []
    for i in range(n):
        dq = dqs[i % len(dqs)]
        nbits = (1 + (i * 7) % 4) * 65536 - (i * 131) % 5000
        out.append(_pair(ctx, P, base + i, dq, nbits, common=(i % 3 == 0)))
    return out


def _check_matrix(P, got, oa, ob, metrics):
    assert got.dtype == np.uint64 and got.shape == (len(metrics), len(oa), len(ob))
    empty = P.new(65536)
    cache = {}
    for i, x in enumerate(oa):
        for j, y in enumerate(ob):
            xx, yy = (x if x is not None else empty), (y if y is not None else empty)
            for k, m in enumerate(metrics):
                key = (id(xx), id(yy), m)
                if key not in cache:
                    cache[key] = _expect(P, xx, yy, m)
                assert int(got[k, i, j]) == cache[key], (i, j, m)


@pytest.fixture(scope="module")
def pool(ctx, port):
    return _pool(ctx, port, 130)


@pytest.mark.parametrize("na,nb", [(1, 1), (3, 17), (17, 3), (70, 1), (1, 130), (70, 130)])
def test_matrix_asymmetric_sizes(ctx, port, pool, na, nb):
    A = pool[:na]
    B = pool[::-1][:nb]
    got = bm.distance_matrix([d for d, _ in A], [d for d, _ in B], (bm.COUNT_AND,))
    _check_matrix(port, got, [o for _, o in A], [o for _, o in B], (bm.COUNT_AND,))


@pytest.mark.parametrize("n", [1, 3, 17, 70, 130])
def test_matrix_symmetric_sizes(ctx, port, pool, n):
    A = pool[:n]
    got = bm.distance_matrix([d for d, _ in A], None, (bm.COUNT_AND, bm.COUNT_A, bm.COUNT_B))
    _check_matrix(port, got, [o for _, o in A], [o for _, o in A], (bm.COUNT_AND, bm.COUNT_A, bm.COUNT_B))


def test_matrix_null_entries_repeats_and_all_metrics(ctx, port, pool):
    A = [pool[0], None, pool[5], pool[5], pool[12], None, pool[0]]
    B = [pool[3], pool[5], None, pool[3], pool[40]]
    dA = [None if p is None else p[0] for p in A]
    dB = [None if p is None else p[0] for p in B]
    oA = [None if p is None else p[1] for p in A]
    oB = [None if p is None else p[1] for p in B]
    got = bm.distance_matrix(dA, dB, ALL)
    _check_matrix(port, got, oA, oB, ALL)
    sym = bm.distance_matrix(dA, None, ALL)
    _check_matrix(port, sym, oA, oA, ALL)


def test_matrix_u64_counts_past_2_32(ctx, port):
    """70,000 FULL blocks (no slab): |F| = 70,000 x 65,536 = 4,587,520,000 > 2^32, against itself and a partial vector"""
    nf = 70000
    F = bm.bvector.from_block_table(ctx, nf * 65536, np.full(nf, bm.FULL, np.uint8), np.zeros(nf, np.uint32),
                                    np.zeros(0, np.uint32), np.zeros(0, np.uint16))
    part = bm.bvector.generate(ctx, SEED, 31, 6554, 3 * 65536 + 7)
    pc = part.count()
    full = nf * 65536
    assert full > 2 ** 32
    got = bm.distance_matrix([F, part], None, ALL)
    exp_and = np.array([[full, pc], [pc, pc]], np.uint64)
    cnt = np.array([full, pc], np.uint64)
    assert (got[0] == exp_and).all()
    assert (got[5] == cnt[:, None]).all() and (got[6] == cnt[None, :]).all()
    assert int(got[1, 0, 1]) == full - pc and int(got[2, 0, 1]) == full and int(got[3, 0, 1]) == full - pc and int(got[4, 0, 1]) == 0
    asym = bm.distance_matrix([F], [F, part], (bm.COUNT_AND, bm.COUNT_OR, bm.COUNT_A, bm.COUNT_B))
    assert asym[:, 0, :].tolist() == [[full, pc], [full, full], [full, full], [full, pc]]
    assert bm.distance_operation(F, F, (bm.COUNT_AND, bm.COUNT_XOR)) == [full, 0]
    assert bm.distance_operation(F, part, (bm.COUNT_AND, bm.COUNT_SUB_AB, bm.COUNT_B)) == [pc, full - pc, pc]


def test_matrix_dev_equals_sync(ctx, port, pool):
    import torch
    A = [d for d, _ in pool[:20]]
    B = [d for d, _ in pool[30:45]]
    exp = bm.distance_matrix(A, B, (bm.COUNT_AND, bm.COUNT_A, bm.COUNT_B))
    d_and = torch.full((len(A) * len(B),), -1, dtype=torch.int64, device="cuda")
    d_ca = torch.full((len(A),), -1, dtype=torch.int64, device="cuda")
    d_cb = torch.full((len(B),), -1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    bm.distance_matrix_dev(A, B, d_and.data_ptr(), d_ca.data_ptr(), d_cb.data_ptr())
    ctx.synchronize()
    assert d_and.cpu().numpy().astype(np.uint64).reshape(len(A), len(B)).tolist() == exp[0].tolist()
    assert d_ca.cpu().numpy().astype(np.uint64).tolist() == exp[1][:, 0].tolist()
    assert d_cb.cpu().numpy().astype(np.uint64).tolist() == exp[2][0, :].tolist()
    # symmetric, AND matrix only; then counts only
    sym = bm.distance_matrix(A, None, (bm.COUNT_AND,))
    d_sym = torch.full((len(A) * len(A),), -1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    bm.distance_matrix_dev(A, None, d_sym.data_ptr())
    ctx.synchronize()
    assert d_sym.cpu().numpy().astype(np.uint64).reshape(len(A), len(A)).tolist() == sym[0].tolist()
    d_ca.fill_(-1)
    torch.cuda.synchronize()
    bm.distance_matrix_dev(A, None, 0, d_ca.data_ptr())
    ctx.synchronize()
    assert d_ca.cpu().numpy().astype(np.uint64).tolist() == [a.count() for a in A]


@pytest.mark.parametrize("members", [[0, 0], [0, 0, 0]])
def test_group_distance_matrix_equals_single_context(ctx, members):
    grp = bm.group(members)
    nbits = 9 * 65536 + 1234
    spec = [(6554, True), (655, False), (66, False), (32768, False), (200, False)]
    ga = [bm.gbvector.generate(grp, SEED, 60 + i, dq, nbits, with_common=c) for i, (dq, c) in enumerate(spec)]
    da = [bm.bvector.generate(ctx, SEED, 60 + i, dq, nbits, with_common=c) for i, (dq, c) in enumerate(spec)]
    got = grp.distance_matrix(ga + [None], ga[1:3], ALL)
    exp = bm.distance_matrix(da + [None], da[1:3], ALL)
    assert got.tolist() == exp.tolist()
    assert grp.distance_matrix(ga, None, ALL).tolist() == bm.distance_matrix(da, None, ALL).tolist()
    del ga
    grp.close()


def test_matrix_equals_pipeline_route_at_1e8_bits(ctx):
    """64 x 1e8 bits, symmetric: the matrix = today's route (a counts-only pipeline, one 2-operand AND group per pair)"""
    n, nbits = 64, 100_000_000
    vs = [bm.bvector.generate(ctx, SEED, 200 + i, 6554 if i % 4 else 655, nbits, with_common=(i % 2 == 0)) for i in range(n)]
    got = bm.distance_matrix(vs, None, (bm.COUNT_AND,))[0]
    pipe = bm.aggregator.pipeline(ctx)
    idx = [(i, j) for i in range(n) for j in range(i, n)]
    for i, j in idx:
        g = pipe.add()
        g.add(vs[i], 0)
        g.add(vs[j], 0)
    pipe.complete()
    cnt = bm.aggregator(ctx).combine_and_sub(pipe)
    for (i, j), c in zip(idx, cnt):
        assert int(got[i, j]) == int(c) and int(got[j, i]) == int(c), (i, j)


_REDZONE_SCRIPT = r'''
import json, os, sys
sys.path.insert(0, os.getcwd())
import bitmagic_amd as bm
ctx = bm.context(0)
out = {"enabled": ctx.redzone_check()["enabled"]}
nbits = 30 * 65536 - 77
vs = [bm.bvector.generate(ctx, 77, i, dq, nbits - i * 9000) for i, dq in enumerate((6554, 655, 66, 30000, 200, 0, 65536, 655))]
m = bm.distance_matrix(vs + [None], None, (6, 7, 8, 9, 10, 11, 12))
m2 = bm.distance_matrix(vs[:3], vs[2:] + [None], (6, 11, 12))
d = bm.distance_operation(vs[1], vs[2], (6, 11, 12))
ctx.synchronize()
out["hits"] = ctx.redzone_check()["hits"]
out["and01"] = int(m[0, 0, 1]); out["pair"] = d
print("REDZONE " + json.dumps(out))
'''


def test_matrix_red_zones_clean():
    """a fresh process under BMX_DEBUG_REDZONE=1: mixed-kind matrices (GAP expansion, tiles, counts) write nothing outside
    their allocations"""
    env = dict(os.environ, BMX_DEBUG_REDZONE="1")
    r = subprocess.run([sys.executable, "-c", _REDZONE_SCRIPT], capture_output=True, text=True, timeout=600, cwd=ROOT, env=env)
    line = [l for l in r.stdout.splitlines() if l.startswith("REDZONE ")]
    assert r.returncode == 0 and line, (r.stdout + r.stderr)[-3000:]
    out = json.loads(line[0][8:])
    assert out["enabled"] and out["hits"] == 0, out


_CPP_CLIENT = r'''
#include "bmx/similarity.hpp"
#include <cstdio>
#include <cstdlib>
#include <memory>

// Jaccard = |A & B| / |A | B| from the batch's (COUNT_AND, COUNT_OR) descriptors
struct jaccard {
    double operator()(const bmx::distance_metric_descriptor* it, const bmx::distance_metric_descriptor* end) const {
        (void)end; return it[1].result ? double(it[0].result) / double(it[1].result) : 0.0;
    }
};

static void fill(bmx::bvector& bv, unsigned seed, unsigned nwords, unsigned density_mask)
{
    std::vector<unsigned> w(nwords);
    unsigned x = seed * 2654435761u + 1u;
    for (unsigned i = 0; i < nwords; ++i) {
        unsigned v = 0;
        for (int k = 0; k < 4; ++k) { x ^= x << 13; x ^= x >> 17; x ^= x << 5; v = (v << 8) ^ (x & 0xFFu); }
        w[i] = ((i / 2048u) % 3u == 1u) ? (v & density_mask & 0x00010001u) : (v & density_mask);   // some sparse (GAP) blocks
    }
    bmx::bit_import_u32(bv, w.data(), nwords, true);
}

#define CHECK(c) do { if (!(c)) { std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); return 1; } } while (0)

int main()
{
    bmx::context ctx(0);
    bmx::bvector a(ctx), b(ctx);
    fill(a, 1, 2048 * 7 + 100, 0xFFFFFFFFu);
    fill(b, 2, 2048 * 5 + 7, 0x0F0F0F0Fu);
    // samples/bvsample09: Dice through ONE distance_operation call; a second call accumulates into result
    bmx::distance_metric_descriptor dmd[3] = {bmx::COUNT_AND, bmx::COUNT_A, bmx::COUNT_B};
    bmx::distance_operation(a, b, dmd, dmd + 3);
    const uint64_t ab = bmx::count_and(a, b), ca = a.count(), cb = b.count();
    CHECK(dmd[0].result == ab && dmd[1].result == ca && dmd[2].result == cb);
    const double dice = 2.0 * double(dmd[0].result) / double(dmd[1].result + dmd[2].result);
    CHECK(dice > 0.0 && dice < 1.0);
    bmx::distance_operation(a, b, dmd, dmd + 3);
    CHECK(dmd[0].result == 2 * ab && dmd[1].result == 2 * ca && dmd[2].result == 2 * cb);
    bmx::distance_metric_descriptor x[2] = {bmx::COUNT_XOR, bmx::COUNT_SUB_BA};
    bmx::distance_operation(a, b, x, x + 2);
    CHECK(x[0].result == bmx::count_xor(a, b) && x[1].result == bmx::count_sub(b, a));

    // a Jaccard batch over slices (one plane absent, one repeated): one matrix call, values = pairwise count_and / count_or
    std::vector<std::unique_ptr<bmx::bvector>> planes;
    for (unsigned i = 0; i < 6; ++i) { planes.emplace_back(new bmx::bvector(ctx)); fill(*planes.back(), 10 + i, 2048 * 3 + 11 * i, i % 2 ? 0x33333333u : 0xFFFF00FFu); }
    std::vector<const bmx::bvector*> slices = {planes[0].get(), planes[1].get(), nullptr, planes[2].get(), planes[3].get(), planes[3].get(),
                                               planes[4].get(), planes[5].get()};
    typedef bmx::similarity_descriptor<bmx::bvector, 2, unsigned, double, jaccard> sd;
    bmx::similarity_batch<sd> batch;
    bmx::build_jaccard_similarity_batch(batch, slices);
    CHECK(batch.descr_vect_.size() == 20);    // 7 present slices, 21 pairs, minus the (3, 3) pair of the repeated plane
    batch.calculate();
    for (auto& d : batch.descr_vect_) {
        const uint64_t and_ = bmx::count_and(*d.get_first(), *d.get_second()), or_ = bmx::count_or(*d.get_first(), *d.get_second());
        CHECK(d.distance_begin()[0].result == and_ && d.distance_begin()[1].result == or_);
        CHECK(d.similarity() == (or_ ? double(and_) / double(or_) : 0.0));
        CHECK(slices[d.get_first_idx()] == d.get_first() && slices[d.get_second_idx()] == d.get_second());
    }
    batch.sort();
    for (size_t k = 1; k < batch.descr_vect_.size(); ++k) CHECK(!(batch.descr_vect_[k] > batch.descr_vect_[k - 1]));
    std::printf("distance client ok\n");
    return 0;
}
'''


def test_cpp_client_dice_and_similarity_batch(tmp_path):
    """a C++ client of bmx::distance_operation (bvsample09's Dice, with the accumulation into result) and of a similarity_batch
    over slices, compiled here against the headers and -lbmx"""
    src = tmp_path / "client.cpp"
    src.write_text(_CPP_CLIENT)
    exe = tmp_path / "client"
    lib = os.path.join(ROOT, "bitmagic_amd", "lib")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), str(src), "-L", lib, "-lbmx",
                    "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib", "-o", str(exe)], check=True)
    env = dict(os.environ)
    env["LD_LIBRARY_PATH"] = lib + ":/opt/rocm/lib:" + env.get("LD_LIBRARY_PATH", "")
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and "distance client ok" in r.stdout, r.stdout + r.stderr
