"""GPU: bm::rank_compressor on the device (src/bmalgo.h:452-707; bmx_rank_compress / bmx_rank_decompress and the _many
forms) against the reference fixture rankc_ref.json, the route composed of the entries that existed before (to_indices ->
rank_batch / select_batch -> from_indices(sorted)), the oracle port and NumPy: block tables byte for byte, sizes, counts and
positions, for both values of optimize, with and without the index, under both values of the tuning key rankc_path."""
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
from rankc_cases import cases, decompress_sources, model_compress, model_decompress, record, sha, words_of  # noqa: E402

with open(os.path.join(GOLDEN, "rankc_ref.json")) as _f:
    FIXTURE = json.load(_f)["cases"]
CASES = cases()
B = 65536
U = np.uint64


@pytest.fixture(params=[0, 1], ids=["positions", "blocks"])
def path(request, ctx):
    ctx.set_tuning("rankc_path", request.param)
    yield request.param
    ctx.set_tuning("rankc_path", -1)


def _vec(ctx, ids, nbits):
    return bm.bvector.from_indices(ctx, np.ascontiguousarray(ids, U), nbits, bm.BM_SORTED, optimize=True)


def _tables_equal(a, b):
    ta, tb = a.block_table(), b.block_table()
    return a.size() == b.size() and all(x.dtype == y.dtype and x.shape == y.shape and (x == y).all() for x, y in zip(ta, tb))


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
    assert v.info()["counts"] == rec["counts"]


def _composed_compress(ctx, idx, rs, src, optimize):
    """the route through the entries the library had before: positions of src & idx, their ranks, a vector of the ranks"""
    ids = bm.bvector.bit_and(src, idx).to_indices()
    ranks = idx.count_to(ids, rs) - U(1) if ids.size else np.zeros(0, U)
    return bm.bvector.from_indices(ctx, ranks, rs.count(), bm.BM_SORTED, optimize)


def _composed_decompress(ctx, idx, rs, src, optimize):
    s = src.to_indices()
    s = s[s < U(rs.count())]
    if s.size:
        found, pos = idx.select(s + U(1), rs)
        assert found.all()
    else:
        pos = np.zeros(0, U)
    return bm.bvector.from_indices(ctx, pos, idx.size(), bm.BM_SORTED, optimize)


@pytest.mark.parametrize("name", sorted(CASES))
def test_fixture_cases(ctx, path, name):
    """every fixture case, both directions, both optimize modes, with and without rs_idx: the reference's table in the device's
    layout, size, count, positions; and the composed route table for table"""
    case, fx = CASES[name], FIXTURE[name]
    rc = bm.rank_compressor(ctx)
    idx = _vec(ctx, case["idx"], case["idx_nbits"])
    src = _vec(ctx, case["src"], case["src_nbits"])
    rs = idx.build_rs_index()
    assert rs.count() == fx["idx_count"]
    dsrc = {k: _vec(ctx, ids, nbits) for k, (ids, nbits) in decompress_sources(name, case).items()}
    for optimize in (False, True):
        okey = "opt1" if optimize else "opt0"
        for use_rs in (False, True):
            got = {"compress": rc.compress_by_source(idx, rs, src, optimize) if use_rs else rc.compress(idx, src, optimize)}
            for k, v in dsrc.items():
                got["decompress_" + k] = rc.decompress(idx, v, rs if use_rs else None, optimize)
            for d, v in got.items():
                c = fx[d]
                _check_table(v, c[okey], c["nbits_out"])
                assert v.count() == c["count"], (name, d, optimize, use_rs)
                ids = v.to_indices()
                assert ids.size == c["count"] and sha(ids.astype("<u8")) == c["ids_sha"], (name, d, optimize, use_rs)
        # the composed route: the same table
        assert _tables_equal(got["compress"], _composed_compress(ctx, idx, rs, src, optimize)), (name, optimize)
        for k, v in dsrc.items():
            assert _tables_equal(got["decompress_" + k], _composed_decompress(ctx, idx, rs, v, optimize)), (name, k, optimize)
    # the round trip gives back src & idx
    back = got["decompress_roundtrip"].to_indices()
    assert (back == np.intersect1d(case["src"], case["idx"])).all()


def _ones(words):
    nz = np.flatnonzero(words)
    bits = np.unpackbits(words[nz].view(np.uint8).reshape(-1, 4), axis=1, bitorder="little")
    wi, bi = np.nonzero(bits)
    return nz[wi].astype(U) * 32 + bi.astype(U)


DENSITIES = {"0.05%": 33, "1%": 655, "10%": 6554, "50%": 32768, "95%": 62259}     # of 65,536


@pytest.mark.parametrize("di", sorted(DENSITIES))
def test_algebra_on_random_vectors(ctx, port, path, di):
    """seeded random vectors of 64 blocks over the density grid: the round-trip identities, the count, and every result against
    the oracle port's rank / select"""
    nbits, seed = 64 * B - 1234, 0x5EED
    rc = bm.rank_compressor(ctx)
    idx = bm.bvector.generate(ctx, seed, 1, DENSITIES[di], nbits)
    pidx = port.import_words(port.gen_words(seed, 1, DENSITIES[di], nbits), True, nbits)
    prs = port.rs_build(pidx)
    rs = idx.build_rs_index()
    cnt = rs.count()
    assert cnt == prs.count()
    for j, ds in enumerate(sorted(DENSITIES)):
        s = bm.bvector.generate(ctx, seed, 10 + j, DENSITIES[ds], nbits)
        ps = port.import_words(port.gen_words(seed, 10 + j, DENSITIES[ds], nbits), True, nbits)
        both = _ones(port.op2(0, ps, pidx).to_words())
        for optimize in (False, True):
            comp = rc.compress(idx, s, optimize)
            exp = prs.rank(both) - U(1) if both.size else np.zeros(0, U)               # count_to(p) - 1 of the port
            assert comp.size() == cnt and comp.count() == bm.count_and(s, idx) == both.size
            assert (comp.to_indices() == exp).all(), (di, ds, optimize)
            assert _tables_equal(comp, _composed_compress(ctx, idx, rs, s, optimize)), (di, ds, optimize)
            back = rc.decompress(idx, comp, rs, optimize)                               # decompress(compress(s)) == s & idx
            assert back.size() == nbits and (back.to_indices() == both).all(), (di, ds, optimize)
            assert bm.count_xor(back, bm.bvector.bit_and(s, idx)) == 0
            # t below count: a generated vector cut to [0, count)
            t_ids = _ones(ps.to_words())
            t_ids = t_ids[t_ids < U(cnt)]
            t = _vec(ctx, t_ids, cnt)
            dec = rc.decompress(idx, t, None, optimize)
            if t_ids.size:
                pos, found = prs.select(t_ids + U(1))
                assert found.all()
            else:
                pos = np.zeros(0, U)
            assert (dec.to_indices() == pos).all(), (di, ds, optimize)
            assert _tables_equal(dec, _composed_decompress(ctx, idx, rs, t, optimize)), (di, ds, optimize)
            again = rc.compress(idx, dec, optimize)                                     # compress(decompress(t)) == t
            assert again.size() == cnt and (again.to_indices() == t_ids).all(), (di, ds, optimize)


def test_defined_extensions(ctx, path):
    """src not a subset of idx: the result of src & idx; src bits at or beyond count(idx): ignored -- against NumPy"""
    rng = np.random.default_rng(77)
    nbits = 5 * B + 100
    idx_ids = np.flatnonzero(rng.random(nbits) < 0.2).astype(U)
    src_ids = np.flatnonzero(rng.random(nbits) < 0.3).astype(U)                         # mostly outside idx
    assert np.setdiff1d(src_ids, idx_ids).size > 0
    idx, src = _vec(ctx, idx_ids, nbits), _vec(ctx, src_ids, nbits)
    rc = bm.rank_compressor(ctx)
    for optimize in (False, True):
        comp = rc.compress(idx, src, optimize)
        assert comp.size() == idx_ids.size and (comp.to_indices() == model_compress(idx_ids, src_ids)).all()
        assert _tables_equal(comp, rc.compress(idx, bm.bvector.bit_and(src, idx), optimize))
        assert (src_ids >= U(idx_ids.size)).any()
        dec = rc.decompress(idx, src, None, optimize)                                   # src reaches far beyond count(idx)
        assert dec.size() == nbits and (dec.to_indices() == model_decompress(idx_ids, src_ids)).all()
        below = _vec(ctx, src_ids[src_ids < U(idx_ids.size)], idx_ids.size)
        assert _tables_equal(dec, rc.decompress(idx, below, None, optimize))
    # a source of one bit exactly at count(idx), and one at count(idx) - 1
    assert rc.decompress(idx, _vec(ctx, [idx_ids.size], nbits)).count() == 0
    assert (rc.decompress(idx, _vec(ctx, [idx_ids.size - 1], nbits)).to_indices() == idx_ids[-1:]).all()


def test_batch_equals_singles(ctx, path):
    """33 sources with absent planes against one index: outs[i] equals the single call table for table; absent -> None"""
    case = CASES["idx_mixed_src_every_kind"]
    idx = _vec(ctx, case["idx"], case["idx_nbits"])
    rs = idx.build_rs_index()
    rng = np.random.default_rng(5)
    pool = [case["src"], CASES["idx_bit"]["src"], CASES["idx_gap"]["src"], np.zeros(0, U), case["idx"]]
    srcs = []
    for i in range(33):
        if i in (3, 17, 32):
            srcs.append(None)
        elif i == 20:
            srcs.append(idx)                                                            # the index's own handle: a copy
        else:
            base = pool[i % len(pool)]
            srcs.append(_vec(ctx, base[rng.random(base.size) < 0.7], 6 * B if i % 2 else 16 * B))
    rc = bm.rank_compressor(ctx)
    for optimize in (False, True):
        for use_rs in (None, rs):
            for many, one in ((rc.compress_many, lambda s: rc.compress_by_source(idx, use_rs, s, optimize)),
                              (rc.decompress_many, lambda s: rc.decompress(idx, s, use_rs, optimize))):
                outs = many(idx, srcs, use_rs, optimize)
                assert len(outs) == 33
                for i, (s, o) in enumerate(zip(srcs, outs)):
                    if s is None:
                        assert o is None, i
                    else:
                        assert _tables_equal(o, one(s)), (i, optimize)
    assert rc.compress_many(idx, []) == [] and rc.decompress_many(idx, [None, None]) == [None, None]


def test_batch_allocation_failure_leaves_nothing(ctx):
    """a failing allocation in the middle of a batch: BMX_ERR_BADALLOC, every outs[i] NULL, bmx_ctx_mem_used unchanged; swept
    over the allocations of the call until it succeeds, for both paths and both directions"""
    case = CASES["idx_bit"]
    idx = _vec(ctx, case["idx"], case["idx_nbits"])
    srcs = [_vec(ctx, case["src"][i::3], case["src_nbits"]) for i in range(3)] + [None, idx]
    n = len(srcs)
    arr = (C.c_void_p * n)(*[(v._h if v is not None else None) for v in srcs])
    L = bm.lib()
    try:
        for p in (0, 1):
            ctx.set_tuning("rankc_path", p)
            for fn in (L.bmx_rank_compress_many, L.bmx_rank_decompress_many):
                ctx.synchronize(); ctx.trim()
                base = ctx.mem_used()
                failed, k = 0, 0
                while True:
                    outs = (C.c_void_p * n)(*([0xDEAD] * n))
                    ctx.inject_failure(4, k)
                    try:
                        rc = fn(ctx._h, idx._h, None, arr, n, 1, outs)
                    finally:
                        ctx.inject_failure(0, 0)
                    ctx.synchronize()
                    if rc == 0:
                        break
                    assert rc == 1, (p, k, rc)
                    assert not any(outs), (p, k)
                    ctx.trim()
                    assert ctx.mem_used() == base, (p, k, ctx.mem_used() - base)
                    failed += 1; k += 1
                    assert k < 400
                assert failed >= 4, (p, failed)                      # the scratch, the layout, and the slabs of more than one output
                res = [bm.bvector(ctx, C.c_void_p(outs[i])) if outs[i] else None for i in range(n)]
                assert res[3] is None and all(r is not None for i, r in enumerate(res) if i != 3)
                del res
                ctx.synchronize(); ctx.trim()
                assert ctx.mem_used() == base
    finally:
        ctx.set_tuning("rankc_path", -1)


def test_identical_handles_give_a_copy(ctx, path):
    """idx == src as handles: a block-for-block copy of src (kinds included), in both directions; the same content under another
    handle is computed: compress gives the run [0, count)"""
    case = CASES["idx_mixed_src_every_kind"]
    idx = _vec(ctx, case["idx"], case["idx_nbits"])
    twin = _vec(ctx, case["idx"], case["idx_nbits"])
    rc = bm.rank_compressor(ctx)
    for fn in (rc.compress, lambda a, b, o: rc.decompress(a, b, None, o)):
        for optimize in (False, True):
            assert _tables_equal(fn(idx, idx, optimize), idx)
    cnt = idx.count()
    comp = rc.compress(idx, twin, True)
    assert comp.size() == cnt and comp.count() == cnt
    assert comp.info()["counts"][bm.FULL] == cnt // B and comp.info()["counts"][bm.BIT] == 0
    assert not _tables_equal(rc.compress(idx, twin, False), idx)


def test_index_argument_errors(ctx):
    """an index of another context, and the index of a vector with another block count: BMX_ERR_BADARG, no output"""
    case = CASES["idx_bit"]
    idx = _vec(ctx, case["idx"], case["idx_nbits"])
    src = _vec(ctx, case["src"], case["src_nbits"])
    other = _vec(ctx, CASES["src_longer"]["src"], 8 * B)
    rs_other = other.build_rs_index()
    c2 = bm.context(0)
    idx2 = _vec(c2, case["idx"], case["idx_nbits"])
    rs2 = idx2.build_rs_index()
    L = bm.lib()
    srcs = (C.c_void_p * 1)(src._h)
    for rs in (rs2, rs_other):
        for fn in (L.bmx_rank_compress, L.bmx_rank_decompress):
            out = C.c_void_p(0xDEAD)
            assert fn(ctx._h, idx._h, rs._h, src._h, 0, C.byref(out)) == 2 and not out.value
        for fn in (L.bmx_rank_compress_many, L.bmx_rank_decompress_many):
            outs = (C.c_void_p * 1)(0xDEAD)
            assert fn(ctx._h, idx._h, rs._h, srcs, 1, 0, outs) == 2 and not outs[0]
    out = C.c_void_p(0xDEAD)
    assert L.bmx_rank_compress(ctx._h, idx2._h, None, src._h, 0, C.byref(out)) == 2 and not out.value    # a foreign index vector
    assert L.bmx_rank_compress(ctx._h, idx._h, None, idx2._h, 0, C.byref(out)) == 2 and not out.value    # a foreign source
    with pytest.raises(bm.BmxError):
        ctx.set_tuning("rankc_path", 2)
    del rs2, idx2
    c2.close()


def test_scanner_decompress(ctx, port):
    """slice_scanner.decompress: a result in rank space through the NOT-NULL vector, against select of the oracle port; without
    a NOT-NULL vector the argument comes back"""
    case = CASES["idx_null_between"]
    not_null = _vec(ctx, case["idx"], case["idx_nbits"])
    cnt = case["idx"].size
    res_ids = np.flatnonzero(np.random.default_rng(3).random(cnt) < 0.1).astype(U)
    res = _vec(ctx, res_ids, cnt)
    sc = bm.slice_scanner(ctx, [], size=case["idx_nbits"], not_null=not_null)
    prs = port.rs_build(port.import_words(words_of(case["idx"], case["idx_nbits"]), True, case["idx_nbits"]))
    pos, found = prs.select(res_ids + U(1))
    assert found.all()
    for rs in (None, not_null.build_rs_index()):
        out = sc.decompress(res, rs)
        assert out.size() == case["idx_nbits"] and (out.to_indices() == pos).all()
    plain = bm.slice_scanner(ctx, [], size=cnt)
    assert plain.decompress(res) is res


_REDZONE_SCRIPT = r'''
import json, os, sys
sys.path.insert(0, os.getcwd())
sys.path.insert(0, os.path.join(os.getcwd(), "tests", "golden"))
import numpy as np
import bitmagic_amd as bm
from rankc_cases import cases, decompress_sources
ctx = bm.context(0)
out = {"enabled": ctx.redzone_check()["enabled"], "counts": {}}
rc = bm.rank_compressor(ctx)
C = cases()
mk = lambda ids, nbits: bm.bvector.from_indices(ctx, np.ascontiguousarray(ids, np.uint64), nbits, bm.BM_SORTED, optimize=True)
for name in sorted(C):
    case = C[name]
    idx, src = mk(case["idx"], case["idx_nbits"]), mk(case["src"], case["src_nbits"])
    rs = idx.build_rs_index()
    ds = {k: mk(ids, nbits) for k, (ids, nbits) in decompress_sources(name, case).items()}
    for path in (0, 1, -1):
        ctx.set_tuning("rankc_path", path)
        for optimize in (False, True):
            for r in (None, rs):
                got = {"compress": rc.compress_by_source(idx, r, src, optimize)}
                for k, v in ds.items():
                    got["decompress_" + k] = rc.decompress(idx, v, r, optimize)
                outs = rc.compress_many(idx, [src, None, src], r, optimize) + rc.decompress_many(idx, [None] + list(ds.values()), r, optimize)
                for d, v in got.items():
                    out["counts"].setdefault(name + "/" + d, set()).add(v.count())
                out["counts"].setdefault(name + "/compress", set()).add(outs[0].count())
                del got, outs
ctx.synchronize()
out["counts"] = {k: sorted(v) for k, v in out["counts"].items()}
out["hits"] = ctx.redzone_check()["hits"]
print("REDZONE " + json.dumps(out))
'''


def test_red_zones_clean():
    """a fresh process under BMX_DEBUG_REDZONE=1: every fixture case through both paths, both directions and the batch entries
    writes nothing outside its allocations"""
    env = dict(os.environ, BMX_DEBUG_REDZONE="1")
    r = subprocess.run([sys.executable, "-c", _REDZONE_SCRIPT], capture_output=True, text=True, timeout=900, cwd=ROOT, env=env)
    line = [l for l in r.stdout.splitlines() if l.startswith("REDZONE ")]
    assert r.returncode == 0 and line, (r.stdout + r.stderr)[-3000:]
    out = json.loads(line[0][8:])
    assert out["enabled"] and out["hits"] == 0, out
    for key, cnts in out["counts"].items():
        name, d = key.split("/")
        assert cnts == [FIXTURE[name][d]["count"]], key
