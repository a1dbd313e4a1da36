"""CPU: the entry points that build a vector from a list of inclusive [left, right] pairs (bvector::set_range per pair on an
empty vector, then optimize(); src/bm.h:2398, 2383, 7908) and that return a vector as its intervals (bm::interval_enumerator,
src/bmintervals.h:52) are declared, exported and typed; their argument checks answer before any device is touched; the Python
surface refuses what it cannot pass on; the facade compiles standalone with the new methods; the oracle port reproduces the
reference fixture range_ref.json case by case."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
ENTRIES = ("bmx_vec_from_ranges", "bmx_vec_from_ranges_dev", "bmx_vec_from_ranges_shard", "bmx_gvec_from_ranges",
           "bmx_vec_to_ranges", "bmx_vec_to_ranges_dev")


def test_entries_declared_exported_and_cited():
    from bitmagic_amd import _ffi
    names = _ffi.exported_symbols()
    L = _ffi.lib()
    hdr = open(os.path.join(ROOT, "include", "bmx.h")).read()
    for e in ENTRIES:
        assert e in names, e
        assert hasattr(L, e) and getattr(L, e).argtypes, e
        assert ("int %s(" % e) in hdr, e
    for cite in ("src/bm.h:2398", "src/bm.h:2407", "src/bmintervals.h:52-226"):
        assert cite in hdr, cite


def test_argument_checks_without_a_device():
    from bitmagic_amd import _ffi
    L = _ffi.lib()
    null = C.c_void_p()
    pairs = (C.c_uint32 * 4)(1, 2, 5, 9)
    out = C.c_void_p()
    BAD, RANGE = _ffi.ERR_BADARG, _ffi.ERR_RANGE
    build = (lambda *a: L.bmx_vec_from_ranges(*a), lambda *a: L.bmx_vec_from_ranges_dev(*a),
             lambda c, p, w, n, nb, o: L.bmx_vec_from_ranges_shard(c, p, w, n, nb, 0, 0xFFFFFFFF, o),
             lambda *a: L.bmx_gvec_from_ranges(*a))
    for f in build:
        for w in (0, 1, 2, 3, 5, 16, -4):                                   # width 4 or 8 only
            assert f(null, pairs, w, 2, 0, C.byref(out)) == BAD
        assert f(null, None, 4, 2, 0, C.byref(out)) == BAD                  # n > 0 with no pairs
        assert f(null, pairs, 4, 2, 0, None) == BAD                         # no out
        assert f(null, pairs, 4, 1 << 32, 0, C.byref(out)) == RANGE         # more than 2^32 - 1 pairs
        assert f(null, pairs, 4, 2, (1 << 36) + 1, C.byref(out)) == RANGE   # beyond 2^20 blocks
        assert f(null, pairs, 8, 1, 0, C.byref(out)) == BAD                 # (valid arguments reach the handle check)
        assert f(null, None, 4, 0, 0, C.byref(out)) == BAD                  # (an empty list is fine: the null handle is not)
    n = C.c_uint64(77)
    buf = (C.c_uint64 * 4)()
    for f in (L.bmx_vec_to_ranges, L.bmx_vec_to_ranges_dev):
        assert f(null, null, 8, buf, 2, C.byref(n)) == BAD                  # no context, no vector
        assert f(null, null, 8, None, 2, C.byref(n)) == BAD                 # cap > 0 without a buffer
        assert f(null, null, 3, buf, 2, C.byref(n)) == BAD
        assert f(null, null, 8, buf, 2, None) == BAD


def test_python_surface():
    import bitmagic_amd as bm
    assert callable(bm.bvector.from_ranges) and callable(bm.gbvector.from_ranges) and callable(bm.bvector.to_ranges)
    for m in ("set_range", "clear_range", "keep_range", "to_ranges_dev"):
        assert callable(getattr(bm.bvector, m))
    for a, w in ((np.array([[1, 2], [5, 9]], np.uint32), 4), (np.array([[1, 2]], np.int32), 4), (np.array([[1, 2]], np.uint64), 8),
                 (np.array([[1, 2]], np.int64), 8), (np.array([[1, 2]], np.uint16), 4), ([[1, 2], [3, 4], [9, 5]], 8),
                 (np.zeros((0, 2), np.uint64), 8), ([], 8)):
        hold, ptr, width, n, dev = bm._ranges_arg(a)
        assert width == w and n == len(a) and not dev and hold.flags["C_CONTIGUOUS"] and hold.size == 2 * n
    with pytest.raises(TypeError):
        bm._ranges_arg(np.array([[1.5, 2.0]]))
    for bad in (np.array([1, 2, 3, 4], np.uint64), np.zeros((2, 3), np.uint64), np.zeros((2, 2, 2), np.uint32), np.zeros((2, 1), np.uint32)):
        with pytest.raises(ValueError):
            bm._ranges_arg(bad)


def test_facade_compiles_standalone(tmp_path):
    src = tmp_path / "f.cpp"
    src.write_text('#include "bmx/bvector.hpp"\n#include "bmx/group.hpp"\n'
                   'int main(){ bmx::context ctx(0); bmx::bvector bv(ctx);\n'
                   '  bv.set_range(10, 70000); bv.set_range(5, 3, false); bv.set_range(1, 2, true).clear_range(100, 200);\n'
                   '  bv.keep_range(0, 65535);\n'
                   '  std::pair<bmx::size_type, bmx::size_type> p[2] = {{1, 5}, {70000, 9}};\n'
                   '  bv.assign_ranges(p, 2); bv.assign_ranges(p, 2, 1000000);\n'
                   '  std::vector<std::pair<bmx::size_type, bmx::size_type>> r; bv.to_ranges(r);\n'
                   '  bmx::device_group g({0}); bmx::gbvector gv(g); gv.assign_ranges(p, 2); gv.assign_ranges(p, 2, 1 << 20);\n'
                   '  return (int)r.size(); }\n')
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)],
                   check=True)


def _fixture():
    with open(os.path.join(GOLDEN, "range_ref.json")) as f:
        return json.load(f)


def test_fixture_is_small_and_complete():
    assert os.path.getsize(os.path.join(GOLDEN, "range_ref.json")) < 100_000
    sys.path.insert(0, GOLDEN)
    from range_cases import cases
    fx = _fixture()["cases"]
    assert sorted(fx) == sorted(cases())
    kinds_seen = set()
    for c in fx.values():
        kinds_seen |= {k for k in range(4) if c["table"]["counts"][k]}
    assert kinds_seen == {0, 1, 2, 3}
    assert fx["runs_1275"]["table"]["counts"] == [1, 0, 0, 1] and fx["runs_1276"]["table"]["counts"] == [1, 0, 1, 0]   # the GAP threshold
    assert fx["union_is_block_2"]["table"]["counts"] == [2, 1, 0, 0] and fx["union_is_block_2"]["intervals"] == 1
    assert fx["across_border"]["intervals"] == 1 and fx["touching"]["intervals"] == 2
    assert fx["every_7_bits"]["table"]["counts"] == [0, 0, 4, 0] and fx["every_7_bits"]["count"] == 112347


def test_runs_of_words():
    """the helper that turns words into intervals, on a vector small enough to check bit by bit"""
    sys.path.insert(0, GOLDEN)
    from range_cases import runs_of_words
    rng = np.random.default_rng(5)
    bits = (rng.random(3 * 65536) < 0.4).astype(np.uint8)
    bits[65530:65540] = 1; bits[0] = 1; bits[-1] = 1; bits[2 * 65536 - 1] = 1; bits[2 * 65536] = 0
    words = np.packbits(bits, bitorder="little").view(np.uint32)
    d = np.diff(np.concatenate([[0], bits.astype(np.int8), [0]]))
    exp = np.stack([np.flatnonzero(d == 1), np.flatnonzero(d == -1) - 1], axis=1).astype(np.uint64)
    assert (runs_of_words(words) == exp).all()
    assert runs_of_words(np.zeros(2048, np.uint32)).shape == (0, 2)


@pytest.mark.parametrize("name", sorted(_fixture()["cases"]))
def test_port_matches_reference_fixture(name, port):
    """P.new(nbits'), set_range per pair, optimize(), flatten: the reference's table; the runs of its words: the intervals.
    Rebuilding from the intervals gives the same table."""
    sys.path.insert(0, GOLDEN)
    from range_cases import cases, oracle_table, record, sha
    pairs, nbits, _ = cases()[name]
    c = _fixture()["cases"][name]
    nbits_out, table, count, runs = oracle_table(port, pairs, nbits)
    assert nbits_out == c["nbits_out"] and count == c["count"]
    assert record(*table) == c["table"], name
    assert runs.shape[0] == c["intervals"] and sha(runs.astype("<u8")) == c["intervals_sha"]
    assert count == int((runs[:, 1] - runs[:, 0] + 1).sum())
    _, table2, count2, _ = oracle_table(port, runs, c["nbits_out"])
    assert record(*table2) == c["table"] and count2 == count


def test_generator_reproduces_fixture_where_the_reference_is_built():
    import oracle
    if not (oracle.have_reference("avx2") and oracle.have_reference("avx2_64")):
        return                                               # (the committed fixture is what the other tests check)
    r = subprocess.run([sys.executable, os.path.join(GOLDEN, "make_range_golden.py"), "--check"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
