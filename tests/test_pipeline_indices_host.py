"""CPU: the entry points that return every arg-group's hits of a pipeline as one CSR of ascending positions
(combine_and_sub(BII bi, ...) src/bmaggregator.h:1226-1284 per group) are declared, exported and typed; their argument checks
answer before any device is touched; the header still compiles as C99; the facades compile standalone with the new methods; the
expected-value helper of the GPU tests agrees between the oracle port and the reference where the reference is built."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
ENTRIES = ("bmx_pipeline_run_indices", "bmx_pipeline_run_indices_dev")


def test_entries_declared_exported_and_cited():
    from bitmagic_amd import _ffi
    names = _ffi.exported_symbols()
    L = _ffi.lib()
    hdr = open(os.path.join(ROOT, "include", "bmx.h")).read()
    for e in ENTRIES:
        assert e in names, e
        assert hasattr(L, e) and getattr(L, e).argtypes, e
        assert ("int %s(" % e) in hdr, e
    nm = subprocess.run(["nm", "-D", "--defined-only", _ffi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for e in ENTRIES:
        assert (" T %s\n" % e) in nm, e
    for cite in ("src/bmaggregator.h:1226-1284", "src/bmsparsevec_algo.h:1096", '"hits_table_kb"', "set_search_count_limit is NOT applied"):
        assert cite in hdr, cite


def test_header_compiles_as_c99(tmp_path):
    src = tmp_path / "h.c"
    src.write_text('#include "bmx.h"\n'
                   'int use(bmx_ctx* c, bmx_pipeline* p, uint64_t* off, void* out, uint64_t* n)\n'
                   '{ return bmx_pipeline_run_indices(c, p, 0u, UINT32_MAX, 8, off, out, 0u, n)\n'
                   '       + bmx_pipeline_run_indices_dev(c, p, 0u, UINT32_MAX, 4, off, (uint64_t*)0, out, 0u, n); }\n')
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)],
                   check=True)


def test_argument_checks_without_a_device():
    from bitmagic_amd import _ffi
    L = _ffi.lib()
    null = C.c_void_p()
    off = (C.c_uint64 * 4)()
    buf = (C.c_uint64 * 4)()
    n = C.c_uint64(77)
    BAD = _ffi.ERR_BADARG
    for w in (8, 4, 3, 0):
        assert L.bmx_pipeline_run_indices(null, null, 0, 0xFFFFFFFF, w, off, buf, 4, C.byref(n)) == BAD         # no context, no pipeline
        assert L.bmx_pipeline_run_indices_dev(null, null, 0, 0xFFFFFFFF, w, off, None, buf, 4, C.byref(n)) == BAD
    assert L.bmx_pipeline_run_indices(null, null, 0, 0xFFFFFFFF, 8, off, buf, 4, None) == BAD


def test_python_surface():
    import bitmagic_amd as bm
    assert callable(bm.aggregator.combine_and_sub_indices) and callable(bm.aggregator.combine_and_sub_indices_dev)
    assert callable(bm.slice_scanner.find_eq_indices)


def test_facades_compile_standalone(tmp_path):
    src = tmp_path / "f.cpp"
    src.write_text('#include "bmx/scanner.hpp"\n'
                   'int main(){ bmx::context ctx(0); bmx::bvector a(ctx), b(ctx);\n'
                   '  bmx::aggregator<> agg(ctx);\n'
                   '  bmx::aggregator<>::pipeline<bmx::agg_opt_only_counts> pipe(ctx);\n'
                   '  bmx::aggregator<>::pipeline<bmx::agg_run_options<false, false, true> > masked(ctx);\n'
                   '  pipe.add()->add(&a, 0); pipe.complete(); masked.add()->add(&b, 0); masked.complete();\n'
                   '  std::vector<bmx::size_type> off, ids;\n'
                   '  agg.combine_and_sub_indices(pipe, off, ids); agg.set_range_hint(5, 70000); agg.combine_and_sub_indices(masked, off, ids);\n'
                   '  bmx::slice_scanner sc(ctx); std::vector<const bmx::bvector*> planes(3, &a); sc.bind(planes);\n'
                   '  uint64_t v[3] = {0, 5, 9}; sc.find_eq_indices(v, 3, off, ids);\n'
                   '  return (int)ids.size(); }\n')
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)],
                   check=True)


def test_expected_value_helper(port):
    """the CSR the GPU tests compare against: offsets are the running sizes, every segment is ascending and inside the columns of
    the run, a column range selects exactly the positions of the full run that lie in it; the reference gives the same arrays"""
    import oracle
    import pipe_indices_cases as pc
    pv = pc.oracle_operands(port)
    groups = pc.grid_groups()
    off, ids = pc.expected_csr(port, pv, groups)
    assert off[0] == 0 and off[-1] == ids.size and off.size == len(groups) + 1
    for g in range(len(groups)):
        seg = ids[int(off[g]):int(off[g + 1])]
        assert (np.diff(seg.astype(np.int64)) > 0).all() and (seg.size == 0 or seg[-1] < pc.NBITS)
    o2, i2 = pc.expected_csr(port, pv, groups, 2, 5)
    parts = [ids[int(off[g]):int(off[g + 1])] for g in range(len(groups))]
    parts = [p[(p >= 2 * pc.B) & (p < 5 * pc.B)] for p in parts]
    assert (i2 == np.concatenate(parts)).all() and (np.diff(o2.astype(np.int64)) == [p.size for p in parts]).all()
    v = port.agg_and_sub([pv[("a", 7)], pv[("a", 8)]], [pv[("s", 1)], pv[("s", 2)]])
    assert int(off[3] - off[2]) == v.count() and all(v.get_bit(int(p)) for p in ids[int(off[2]):int(off[2]) + 50])
    if oracle.have_reference("avx2"):
        R = oracle.reference("avx2")
        rv = pc.oracle_operands(R)
        for grp in (groups, pc.chunk_groups()[:20]):
            a, b = pc.expected_csr(R, rv, grp), pc.expected_csr(port, pv, grp)
            assert (a[0] == b[0]).all() and (a[1] == b[1]).all()
