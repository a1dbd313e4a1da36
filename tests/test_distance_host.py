"""CPU: the distance entry points (bm::distance_operation, src/bmalgo_impl.h:766, and the all-pairs matrices) are declared,
exported and typed; their argument checks answer before any device is touched; the metric codes are the reference's; the
similarity header is plain C++17."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("bmx_distance", "bmx_distance_matrix", "bmx_distance_matrix_dev", "bmx_gdistance_matrix")


def test_entries_declared_exported_and_cited():
    from bitmagic_amd import _ffi
    names = _ffi.exported_symbols()
    L = _ffi.lib()
    for e in ENTRIES:
        assert e in names, e
        assert hasattr(L, e) and getattr(L, e).argtypes, e
    hdr = open(os.path.join(ROOT, "include", "bmx.h")).read()
    assert "src/bmalgo_impl.h:766" in hdr


def test_metric_codes_are_the_reference_values():
    """bm::distance_metric = set_operation codes (src/bmconst.h:175-182: COUNT_AND = 6 ... COUNT_B = 12)"""
    import bitmagic_amd as bm
    exp = {"AND": 6, "XOR": 7, "OR": 8, "SUB_AB": 9, "SUB_BA": 10, "A": 11, "B": 12}
    hdr = open(os.path.join(ROOT, "include", "bmx.h")).read()
    for k, v in exp.items():
        assert getattr(bm, "COUNT_" + k) == v
        assert re.search(r"#define BMX_COUNT_%s\s+%d\b" % (k, v), hdr), k
    cpp = open(os.path.join(ROOT, "include", "bmx", "bvector.hpp")).read()
    for k, v in exp.items():
        assert re.search(r"COUNT_%s\s*=\s*BMX_COUNT_%s" % (k, k), cpp), k


def _ints(*v):
    return (C.c_int * len(v))(*v)


def test_argument_checks_without_a_device():
    from bitmagic_amd import _ffi
    L = _ffi.lib()
    null = C.c_void_p()
    res = (C.c_uint64 * 8)()
    one = (C.c_void_p * 1)()
    # bad metric codes
    for bad in (0, 5, 13, -1):
        assert L.bmx_distance(null, null, null, _ints(6, bad), 2, res) == _ffi.ERR_BADARG
        assert L.bmx_distance_matrix(null, one, 1, None, 0, _ints(bad), 1, res) == _ffi.ERR_BADARG
        assert L.bmx_gdistance_matrix(null, one, 1, None, 0, _ints(bad), 1, res) == _ffi.ERR_BADARG
    assert L.bmx_distance(null, null, null, None, 0, res) == _ffi.ERR_BADARG
    # null outputs / lists
    assert L.bmx_distance(null, null, null, _ints(6), 1, None) == _ffi.ERR_BADARG
    assert L.bmx_distance_matrix(null, one, 1, None, 0, _ints(6), 1, None) == _ffi.ERR_BADARG
    assert L.bmx_distance_matrix(null, None, 3, None, 0, _ints(6), 1, res) == _ffi.ERR_BADARG
    assert L.bmx_gdistance_matrix(null, one, 1, None, 0, _ints(6), 1, None) == _ffi.ERR_BADARG
    # list sizes
    for na, nb in ((65536, 1), (1, 65536), (100000, 0)):
        big = (C.c_void_p * max(na, nb))()
        b = big if nb else None
        assert L.bmx_distance_matrix(null, big, na, b, nb, _ints(6), 1, res) == _ffi.ERR_RANGE
        assert L.bmx_distance_matrix_dev(null, big, na, b, nb, None, None, None) == _ffi.ERR_RANGE
        assert L.bmx_gdistance_matrix(null, big, na, b, nb, _ints(6), 1, res) == _ffi.ERR_RANGE
    assert L.bmx_distance_matrix_dev(null, one, 1, None, 0, None, None, None) == _ffi.ERR_BADARG


def test_python_surface():
    import bitmagic_amd as bm
    for n in ("distance_operation", "distance_matrix", "distance_matrix_dev", "COUNT_AND", "COUNT_B"):
        assert n in bm.__all__ and hasattr(bm, n)
    assert callable(bm.group.distance_matrix)
    out = bm.distance_matrix([], None, (bm.COUNT_AND, bm.COUNT_OR))
    assert out.shape == (2, 0, 0) and out.dtype.name == "uint64"


def test_similarity_header_compiles_standalone(tmp_path):
    src = tmp_path / "s.cpp"
    src.write_text('#include "bmx/similarity.hpp"\n'
                   'int main(){ bmx::similarity_batch<bmx::similarity_descriptor<bmx::bvector, 2, double, unsigned, unsigned>> b;\n'
                   '  return (int)b.size(); }\n')
    subprocess.run(["g++", "-std=c++17", "-Wall", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)], check=True)
    bare = tmp_path / "t.cpp"
    bare.write_text('#include "bmx/similarity.hpp"\n')
    subprocess.run(["g++", "-std=c++17", "-Wall", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(bare)], check=True)
