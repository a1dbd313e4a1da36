"""CPU: the entry points that build a vector from a list of bit positions (bvector::set(ids, n, sort_order) on an empty vector,
src/bm.h:4153, 4312, 4364, 4430) are declared, exported and typed; their argument checks answer before any device is touched;
the sort-order codes are the reference's; the facade compiles standalone with the new methods; the oracle port reproduces the
reference fixture import_ref.json case by case."""
import ctypes as C
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
ENTRIES = ("bmx_vec_from_indices", "bmx_vec_from_indices_dev", "bmx_vec_from_indices_shard", "bmx_gvec_from_indices")


def test_entries_declared_exported_and_cited():
    from bitmagic_amd import _ffi
    names = _ffi.exported_symbols()
    L = _ffi.lib()
    for e in ENTRIES:
        assert e in names, e
        assert hasattr(L, e) and getattr(L, e).argtypes, e
    hdr = open(os.path.join(ROOT, "include", "bmx.h")).read()
    assert "src/bm.h:4153,4312,4364,4430" in hdr


def test_sort_order_codes_are_the_reference_values():
    """bm::sort_order (src/bmconst.h:204-210): BM_UNSORTED 0, BM_SORTED 1, BM_SORTED_UNIFORM 2, BM_UNKNOWN 3"""
    import bitmagic_amd as bm
    exp = {"UNSORTED": 0, "SORTED": 1, "SORTED_UNIFORM": 2, "UNKNOWN": 3}
    hdr = open(os.path.join(ROOT, "include", "bmx.h")).read()
    cpp = open(os.path.join(ROOT, "include", "bmx", "bvector.hpp")).read()
    for k, v in exp.items():
        assert getattr(bm, "BM_" + k) == v and "BM_" + k in bm.__all__
        assert re.search(r"#define BMX_%s\s+%d\b" % (k, v), hdr), k
        assert re.search(r"BM_%s\s*=\s*BMX_%s\b" % (k, k), cpp), k


def test_argument_checks_without_a_device():
    from bitmagic_amd import _ffi
    L = _ffi.lib()
    null = C.c_void_p()
    ids = (C.c_uint32 * 4)(1, 2, 3, 4)
    out = C.c_void_p()
    BAD, RANGE = _ffi.ERR_BADARG, _ffi.ERR_RANGE
    host = (lambda *a: L.bmx_vec_from_indices(*a), lambda *a: L.bmx_vec_from_indices_dev(*a),
            lambda c, i, w, n, so, nb, opt, o: L.bmx_vec_from_indices_shard(c, i, w, n, so, nb, 0, 0xFFFFFFFF, opt, o),
            lambda *a: L.bmx_gvec_from_indices(*a))
    for f in host:
        for w in (0, 1, 2, 3, 5, 16, -4):                                   # width 4 or 8 only
            assert f(null, ids, w, 4, 0, 0, 0, C.byref(out)) == BAD
        assert f(null, None, 4, 4, 0, 0, 0, C.byref(out)) == BAD            # n > 0 with no ids
        for so in (-1, 4, 99):                                              # not a bm::sort_order
            assert f(null, ids, 4, 4, so, 0, 0, C.byref(out)) == BAD
        assert f(null, ids, 4, 4, 0, 0, 0, None) == BAD                     # no out
        assert f(null, ids, 4, 1 << 32, 0, 0, 0, C.byref(out)) == RANGE     # more than 2^32 - 1 ids
        for so in (0, 1, 2, 3):                                             # every valid order reaches the handle check
            assert f(null, ids, 8, 4, so, 0, 0, C.byref(out)) == BAD
        assert f(null, None, 4, 0, 3, 0, 0, C.byref(out)) == BAD            # (an empty list is fine: the null handle is not)
    for f in host:
        assert f(null, ids, 4, 4, 0, (1 << 36) + 1, 0, C.byref(out)) == RANGE    # beyond 2^20 blocks
    assert L.bmx_vec_from_indices_shard(null, ids, 4, 4, 0, 0, 0, 0, 0, None) == BAD


def test_python_surface():
    import bitmagic_amd as bm
    assert callable(bm.bvector.from_indices) and callable(bm.gbvector.from_indices)
    for m in ("set", "keep", "clear"):
        assert callable(getattr(bm.bvector, m))
    # the id lists the host entry receives: 32- and 64-bit integers as they are, other integers widened, floats refused
    for a, w in ((np.array([1, 2], np.uint32), 4), (np.array([1, 2], np.int32), 4), (np.array([1, 2], np.uint64), 8),
                 (np.array([1, 2], np.int64), 8), (np.array([1, 2], np.uint16), 4), ([1, 2], 8), ([], 8)):
        hold, ptr, width, n, dev = bm._ids_arg(a)
        assert width == w and n == len(a) and not dev and hold.flags["C_CONTIGUOUS"]
    with pytest.raises(TypeError):
        bm._ids_arg(np.array([1.5]))


def test_facade_compiles_standalone(tmp_path):
    src = tmp_path / "f.cpp"
    src.write_text('#include "bmx/bvector.hpp"\n#include "bmx/group.hpp"\n'
                   'int main(){ bmx::context ctx(0); bmx::bvector bv(ctx);\n'
                   '  bmx::size_type a[3] = {1, 5, 70000}; uint32_t b[2] = {3, 4};\n'
                   '  bv.set(a, 3, bmx::BM_SORTED); bv.set(b, 2); bv.keep(a, 3); bv.keep(b, 2, bmx::BM_UNSORTED);\n'
                   '  bv.clear(a, 3); bv.clear(b, 2, bmx::BM_UNKNOWN); bv.import_sorted(a, 3, true); bv.set(a, 3);\n'
                   '  bmx::device_group g({0}); bmx::gbvector gv(g); gv.assign_indices(a, 3); gv.assign_indices(b, 2, bmx::BM_SORTED, 0, true);\n'
                   '  bmx::sort_order so = bmx::BM_UNKNOWN; return (int)so - 3; }\n')
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)],
                   check=True)


def _fixture():
    with open(os.path.join(GOLDEN, "import_ref.json")) as f:
        return json.load(f)


def test_fixture_is_small_and_complete():
    assert os.path.getsize(os.path.join(GOLDEN, "import_ref.json")) < 100_000
    sys.path.insert(0, GOLDEN)
    from import_cases import cases
    fx = _fixture()["cases"]
    assert sorted(fx) == sorted(cases())
    kinds_seen = set()
    for c in fx.values():
        for opt in ("opt0", "opt1"):
            kinds_seen |= {k for k in range(4) if c[opt]["counts"][k]}
    assert kinds_seen == {0, 1, 2, 3}
    assert fx["runs_1275"]["opt1"]["counts"][3] == 1 and fx["runs_1276"]["opt1"]["counts"][2] == 1     # the GAP threshold
    assert fx["full_block"]["opt1"]["counts"][1] == 1 and fx["full_block"]["opt0"]["counts"][1] == 0     # FULL only under optimize


@pytest.mark.parametrize("name", sorted(_fixture()["cases"]))
def test_port_matches_reference_fixture(name, port):
    """P.new(nbits'), set_bit per id, optimize() when asked, flatten: the reference's tables"""
    sys.path.insert(0, GOLDEN)
    from import_cases import cases, oracle_table, record
    ids, nbits, _ = cases()[name]
    c = _fixture()["cases"][name]
    for opt in (0, 1):
        nbits_out, table, count = oracle_table(port, ids, nbits, bool(opt))
        assert nbits_out == c["nbits_out"] and count == c["count"]
        assert record(*table) == c[f"opt{opt}"], (name, opt)


def test_generator_reproduces_fixture_where_the_reference_is_built():
    import oracle
    if not (oracle.have_reference("avx2") and oracle.have_reference("avx2_64")):
        return                                               # (the committed fixture is what the other tests check)
    r = subprocess.run([sys.executable, os.path.join(GOLDEN, "make_import_golden.py"), "--check"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
