"""bmx::slice_scanner::find_range_counts / histogram (include/bmx/scanner.hpp) from C++.  GPU: against a row loop over the values
the oracle's planes spell and against the loop of count(BMX_CMP_RANGE) calls; the test builds the program with its own compiler
command and runs it once.  CPU: the new methods of both scanners (one device, device group) compile from the facade headers alone."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "bitmagic_amd", "lib")


@pytest.mark.gpu
def test_cpp_range_counts_on_gpu(tmp_path):
    obj, exe = str(tmp_path / "bmx_oracle.o"), str(tmp_path / "test_range_counts")
    subprocess.run(["gcc", "-O2", "-std=c99", "-c", os.path.join(ROOT, "oracle", "bmx_oracle.c"), "-o", obj], check=True, timeout=300)
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "test_range_counts.cpp"), obj, "-o", exe, "-L", LIBDIR, "-lbmx",
                    "-Wl,-rpath," + LIBDIR, "-Wl,-rpath,/opt/rocm/lib"], check=True, timeout=300)
    env = dict(os.environ)
    env["LD_LIBRARY_PATH"] = LIBDIR + ":/opt/rocm/lib:" + env.get("LD_LIBRARY_PATH", "")
    r = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "test_range_counts ok" in r.stdout, r.stdout + r.stderr


def test_facade_methods_compile_alone(tmp_path):
    """CPU: find_range_counts and histogram of slice_scanner and gslice_scanner need nothing but the C header and the facade headers"""
    src = tmp_path / "t.cpp"
    src.write_text('#include "bmx/scanner.hpp"\n#include "bmx/group.hpp"\n'
                   'void f(bmx::slice_scanner& s, bmx::gslice_scanner& g, const bmx::slice_scanner::value_type* v, uint64_t* c)\n'
                   '{ s.find_range_counts(v, v, 3, c); s.histogram(v, 4, c); g.find_range_counts(v, v, 3, c); g.histogram(v, 4, c); }\n'
                   'int main(){return 0;}\n')
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)], check=True)
