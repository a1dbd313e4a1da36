"""CPU: bm::rank_compressor on the device (src/bmalgo.h:452-707) -- the four entries are declared, exported and typed; their
argument checks answer before any device is touched; the Python class and the C++ facade exist and compile; the reference
fixture rankc_ref.json reproduces from the oracle port (rank / select + set_bit + optimize + flatten) and from a NumPy
cumulative-sum model, case by case; where the reference is built, the generator reproduces the committed file."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, GOLDEN)
ENTRIES = ("bmx_rank_compress", "bmx_rank_decompress", "bmx_rank_compress_many", "bmx_rank_decompress_many")
DIRECTIONS = ("compress", "decompress_roundtrip", "decompress_random")


def _fixture():
    with open(os.path.join(GOLDEN, "rankc_ref.json")) as f:
        return json.load(f)


def test_entries_declared_exported_and_cited():
    from bitmagic_amd import _ffi
    names = _ffi.exported_symbols()
    L = _ffi.lib()
    hdr = open(os.path.join(ROOT, "include", "bmx.h")).read()
    for e in ENTRIES:
        assert e in names, e
        assert hasattr(L, e) and getattr(L, e).argtypes, e
        assert ("int %s(" % e) in hdr, e
    assert len(L.bmx_rank_compress.argtypes) == 6 and len(L.bmx_rank_compress_many.argtypes) == 7
    for cite in ("src/bmalgo.h:452-707", ":526-527", ":505-509", "src/bmsparsevec_compr.h:1496", '"rankc_path"'):
        assert cite in hdr, cite


def test_argument_checks_without_a_device():
    from bitmagic_amd import _ffi
    L = _ffi.lib()
    null, out = C.c_void_p(), C.c_void_p(5)
    BAD = _ffi.ERR_BADARG
    for f in (L.bmx_rank_compress, L.bmx_rank_decompress):
        assert f(null, null, null, null, 0, C.byref(out)) == BAD and not out.value      # the output is cleared first
        assert f(null, null, null, null, 0, None) == BAD
        out = C.c_void_p(5)
    outs = (C.c_void_p * 3)(1, 2, 3)
    srcs = (C.c_void_p * 3)()
    for f in (L.bmx_rank_compress_many, L.bmx_rank_decompress_many):
        assert f(null, null, null, srcs, 3, 0, outs) == BAD and not any(outs)
        assert f(null, null, null, srcs, 3, 0, None) == BAD
        assert f(null, null, null, None, 3, 0, outs) == BAD
        outs = (C.c_void_p * 3)(1, 2, 3)


def test_python_surface():
    import bitmagic_amd as bm
    assert "rank_compressor" in bm.__all__
    for m in ("compress", "decompress", "compress_by_source", "compress_many", "decompress_many"):
        assert callable(getattr(bm.rank_compressor, m))
    assert callable(bm.slice_scanner.decompress)
    import inspect
    assert list(inspect.signature(bm.rank_compressor.compress_by_source).parameters)[1:4] == ["bv_idx", "rs_idx", "bv_src"]
    # without a NOT-NULL vector the scanner hands the argument back: the reference's non-compressed branch
    sc = bm.slice_scanner.__new__(bm.slice_scanner)
    sc.not_null = None
    marker = object()
    assert sc.decompress(marker) is marker


def test_facade_compiles_standalone(tmp_path):
    src = tmp_path / "f.cpp"
    src.write_text('#include "bmx/rank_compressor.hpp"\n#include "bmx/bvector.hpp"\n'
                   'int main(){ bmx::context ctx(0); bmx::bvector idx(ctx), src(ctx), t(ctx);\n'
                   '  bmx::rank_compressor rc; bmx::rs_index rs; idx.build_rs_index(&rs);\n'
                   '  rc.compress(t, idx, src); rc.compress(t, idx, src, true);\n'
                   '  rc.decompress(t, idx, src); rc.decompress(t, idx, src, &rs, true);\n'
                   '  rc.compress_by_source(t, idx, rs, src);\n'
                   '  std::vector<bmx::bvector> out; std::vector<const bmx::bvector*> in = {&src, nullptr};\n'
                   '  rc.compress_many(out, idx, in); rc.decompress_many(out, idx, in, &rs, true);\n'
                   '  return (int)out.size(); }\n')
    subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), str(src)],
                   check=True)


def test_fixture_is_small_and_complete():
    assert os.path.getsize(os.path.join(GOLDEN, "rankc_ref.json")) < 100_000
    from rankc_cases import cases
    fx = _fixture()["cases"]
    cs = cases()
    assert sorted(fx) == sorted(cs) and len(cs) == 16
    kinds = {d: set() for d in DIRECTIONS}
    for c in fx.values():
        for d in DIRECTIONS:
            kinds[d] |= {k for k in range(4) if c[d]["opt1"]["counts"][k]}
            assert c[d]["opt0"]["counts"][1] == 0 and c[d]["opt0"]["counts"][3] == 0       # without optimize: NULL or bit-blocks
    assert kinds["compress"] == kinds["decompress_roundtrip"] == {0, 1, 2, 3}, kinds    # every block kind comes out
    assert kinds["decompress_random"] >= {0, 2, 3}, kinds                                 # (a 30 % subset fills no block)
    assert fx["runs_1275"]["compress"]["opt1"]["counts"] == [1, 0, 0, 1]                  # the GAP threshold, both sides
    assert fx["runs_1276"]["compress"]["opt1"]["counts"] == [1, 0, 1, 0]
    assert fx["empty_idx"]["compress"]["nbits_out"] == 0 and fx["empty_src"]["compress"]["count"] == 0
    e = fx["src_equals_idx"]                                                               # the run [0, count)
    assert e["compress"]["count"] == e["idx_count"] == e["compress"]["nbits_out"]
    assert e["compress"]["opt1"]["counts"][1] == e["idx_count"] // 65536
    assert fx["beyond_2_32"]["flavour"] == "avx2_64" and fx["beyond_2_32"]["idx_nbits"] > 1 << 32
    s = fx["sparse_index_many_to_one"]
    assert s["compress"]["opt0"]["nblocks"] == 2 and s["idx_count"] < 24 * 3300           # ~20 index blocks per target block
    d = cs["dense_unaligned_prefix"]
    assert int((d["idx"] < 65536).sum()) % 65536 != 0                                      # index block 1 feeds target blocks 0 and 1
    for name, c in fx.items():                                                             # the round trip gives back src & idx
        both = np.intersect1d(cs[name]["src"], cs[name]["idx"])
        assert c["decompress_roundtrip"]["count"] == c["compress"]["count"] == both.size, name


@pytest.mark.parametrize("name", sorted(_fixture()["cases"]))
def test_port_matches_reference_fixture(name, port):
    from rankc_cases import cases, oracle_case
    assert oracle_case(port, name, cases()[name]) == _fixture()["cases"][name]


@pytest.mark.parametrize("name", sorted(_fixture()["cases"]))
def test_cumulative_sum_model_matches_reference_fixture(name):
    """no oracle at all: positions from searchsorted / indexing, tables from the storage rule"""
    from rankc_cases import cases, decompress_sources, model_case, model_compress, model_decompress, table_of_positions
    case = cases()[name]
    c = _fixture()["cases"][name]
    m = model_case(name, case)
    for d in DIRECTIONS:
        for k in ("nbits_out", "count", "ids_sha"):
            assert m[d][k] == c[d][k], (name, d, k)
    pos = {"compress": model_compress(case["idx"], case["src"])}
    for k, (ids, _) in decompress_sources(name, case).items():
        pos["decompress_" + k] = np.sort(model_decompress(case["idx"], ids))
    for d in DIRECTIONS:
        assert table_of_positions(pos[d], c[d]["nbits_out"], False) == c[d]["opt0"], (name, d)
        assert table_of_positions(pos[d], c[d]["nbits_out"], True) == c[d]["opt1"], (name, d)
    back = np.sort(model_decompress(case["idx"], pos["compress"]))
    assert (back == np.intersect1d(case["src"], case["idx"])).all()


def test_generator_reproduces_fixture_where_the_reference_is_built():
    import oracle
    if not (oracle.have_reference("avx2") and oracle.have_reference("avx2_64")):
        return                                               # (the committed fixture is what the other tests check)
    r = subprocess.run([sys.executable, os.path.join(GOLDEN, "make_rankc_golden.py"), "--check"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
