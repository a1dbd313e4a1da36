"""bmx::set2set_11_transform and bmx::slice_scanner::values (include/bmx/sv_algo.hpp, include/bmx/scanner.hpp) from C++ on the GPU,
against plain loops over the words of vectors of the C oracle; the test builds the program with its own compiler command and runs
it once."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "bitmagic_amd", "lib")


@pytest.mark.gpu
def test_cpp_set2set_on_gpu(tmp_path):
    obj, exe = str(tmp_path / "bmx_oracle.o"), str(tmp_path / "test_set2set")
    subprocess.run(["gcc", "-O2", "-std=c99", "-c", os.path.join(ROOT, "oracle", "bmx_oracle.c"), "-o", obj], check=True, timeout=300)
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "test_set2set.cpp"), obj, "-o", exe, "-L", LIBDIR, "-lbmx",
                    "-Wl,-rpath," + LIBDIR, "-Wl,-rpath,/opt/rocm/lib"], check=True, timeout=300)
    env = dict(os.environ)
    env["LD_LIBRARY_PATH"] = LIBDIR + ":/opt/rocm/lib:" + env.get("LD_LIBRARY_PATH", "")
    r = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "test_set2set ok" in r.stdout, r.stdout + r.stderr
