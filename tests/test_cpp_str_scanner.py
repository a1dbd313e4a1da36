"""bmx::str_scanner (include/bmx/str_scanner.hpp) from C++ on the GPU, against plain loops over the strings; the test builds the
program with its own compiler command and runs it once."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "bitmagic_amd", "lib")


@pytest.mark.gpu
def test_cpp_str_scanner_on_gpu(tmp_path):
    exe = str(tmp_path / "test_str_scanner")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "test_str_scanner.cpp"), "-o", exe, "-L", LIBDIR, "-lbmx",
                    "-Wl,-rpath," + LIBDIR, "-Wl,-rpath,/opt/rocm/lib"], check=True, timeout=300)
    env = dict(os.environ)
    env["LD_LIBRARY_PATH"] = LIBDIR + ":/opt/rocm/lib:" + env.get("LD_LIBRARY_PATH", "")
    r = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "test_str_scanner ok" in r.stdout, r.stdout + r.stderr
