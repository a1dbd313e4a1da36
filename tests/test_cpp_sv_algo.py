"""bmx::sparse_vector_find_mismatch / _count_mismatch / _find_first_mismatch (include/bmx/sv_algo.hpp) from C++.  GPU: against word
loops over vectors of the C oracle; the test builds the program with its own compiler command and runs it once.  CPU: the overloads
of bm_adapter.hpp over two host bm::sparse_vector<> compile against the unmodified reference headers where those exist (compile
check only: the reference headers and a GPU are never on one machine)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "bitmagic_amd", "lib")
REF = "/root/reference/src"


@pytest.mark.gpu
def test_cpp_sv_algo_on_gpu(tmp_path):
    obj, exe = str(tmp_path / "bmx_oracle.o"), str(tmp_path / "test_sv_algo")
    subprocess.run(["gcc", "-O2", "-std=c99", "-c", os.path.join(ROOT, "oracle", "bmx_oracle.c"), "-o", obj], check=True, timeout=300)
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "test_sv_algo.cpp"), obj, "-o", exe, "-L", LIBDIR, "-lbmx",
                    "-Wl,-rpath," + LIBDIR, "-Wl,-rpath,/opt/rocm/lib"], check=True, timeout=300)
    env = dict(os.environ)
    env["LD_LIBRARY_PATH"] = LIBDIR + ":/opt/rocm/lib:" + env.get("LD_LIBRARY_PATH", "")
    r = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "test_sv_algo ok" in r.stdout, r.stdout + r.stderr


def test_facade_header_compiles_alone(tmp_path):
    """CPU: sv_algo.hpp needs nothing but the C header and the facade headers"""
    src = tmp_path / "t.cpp"
    src.write_text('#include "bmx/sv_algo.hpp"\n'
                   'bool f(bmx::bvector& bv, const bmx::slice_scanner& a, const bmx::slice_scanner& b, bmx::size_type& i)\n'
                   '{ bmx::sparse_vector_find_mismatch(bv, a, b, bmx::no_null); return bmx::sparse_vector_find_first_mismatch(a, b, i)\n'
                   '  && bmx::sparse_vector_count_mismatch(a, b, bmx::use_null) != 0; }\nint main(){return 0;}\n')
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)], check=True)


def test_adapter_overloads_compile_against_reference(tmp_path):
    """CPU, where the reference headers exist: the overloads over two host bm::sparse_vector<> with the reference's argument order"""
    if not os.path.exists(os.path.join(REF, "bmsparsevec.h")):
        return                                               # (nothing to compile against)
    src = tmp_path / "t.cpp"
    src.write_text('#include "bm.h"\n#include "bmsparsevec.h"\n#include "bmx/bm_adapter.hpp"\n'
                   'typedef bm::sparse_vector<unsigned, bm::bvector<> > sv_t;\n'
                   'bool f(bmx::context& c, bm::bvector<>& bv, const sv_t& a, const sv_t& b, sv_t::size_type& i)\n'
                   '{ bmx::sparse_vector_find_mismatch(c, bv, a, b, bm::no_null);\n'
                   '  return bmx::sparse_vector_find_first_mismatch(c, a, b, i) && bmx::sparse_vector_find_first_mismatch(c, a, b, i, bm::no_null); }\n'
                   'int main(){return 0;}\n')
    subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-I", REF, "-I", os.path.join(ROOT, "include"), str(src)], check=True)
