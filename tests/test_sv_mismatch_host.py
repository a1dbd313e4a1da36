"""CPU: the reference fixture of bm::sparse_vector_find_mismatch / sparse_vector_find_first_mismatch
(src/bmsparsevec_algo.h:656-792, 478-636) over two bit-sliced columns: sv_mismatch_ref.json reproduces from the oracle port driven
through the reference's own sequence of whole-vector calls and from a NumPy model on the rows' values, case by case; where the
reference is built, the generator reproduces the committed file; the library exports the two entries and refuses a null context."""
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
B = 65536


def _fixture():
    with open(os.path.join(GOLDEN, "sv_mismatch_ref.json")) as f:
        return json.load(f)


def test_fixture_is_small_and_complete():
    assert os.path.getsize(os.path.join(GOLDEN, "sv_mismatch_ref.json")) < 100_000
    from sv_mismatch_cases import K_BIT, K_FULL, K_GAP, K_NULL, case_size, cases, has_vector_result, PROCS
    fx = _fixture()["cases"]
    cs = cases()
    assert sorted(fx) == sorted(cs) and len(cs) == 34
    assert max(case_size(c) for c in cs.values()) <= 64 * B
    # the grid: column c holds the kinds (c & 3, c >> 2) in (A_0, B_0) and the transposed pair in plane 1
    g = cs["grid"]
    assert case_size(g) == 16 * B - 77
    for key, shift in (("a0", 0), ("b0", 2), ("a1", 2), ("b1", 0)):
        held = np.bincount((g["vecs"][key][0] >> np.uint64(16)).astype(np.int64), minlength=16)
        for c in range(16):
            kind = (c >> shift) & 3
            assert (held[c] == 0) == (kind == K_NULL) and (held[c] >= B - 77) == (kind == K_FULL), (key, c)
    assert {K_NULL, K_FULL, K_GAP, K_BIT} == {0, 1, 2, 3}
    # use_null without any not-NULL vector has no vector result, and only that
    for name, c in cs.items():
        for pname, proc in PROCS.items():
            assert (fx[name][pname]["count"] is None) == (not has_vector_result(c, proc)), (name, pname)
            assert (fx[name][pname]["ids_sha"] is None) == (fx[name][pname]["count"] is None)
        assert fx[name]["size"] == case_size(c)
    assert fx["grid"]["use_null"]["count"] is None and fx["grid"]["use_null"]["first"][0]
    assert [len(cs["ragged_5_9"][s]["planes"]) for s in "ab"] == [5, 9] and None in cs["ragged_5_9"]["a"]["planes"] and None in cs["ragged_5_9"]["b"]["planes"]
    assert len(cs["planes_64"]["a"]["planes"]) == 64 and case_size(cs["planes_64"]) <= B
    assert len(cs["values_32"]["a"]["planes"]) == 32 and case_size(cs["values_32"]) == 3 * B - 1000
    assert (cs["size_in_block_both"]["a"]["size"], cs["size_in_block_both"]["b"]["size"]) == (B + 100, B + 5000)
    assert (cs["size_across_both"]["a"]["size"], cs["size_across_both"]["b"]["size"]) == (B - 3, 4 * B + 17)
    for n in ("same_handles", "equal_gap_vs_bit", "size_zero", "no_planes"):
        for p in PROCS:
            assert fx[n][p]["count"] == 0 and fx[n][p]["first"] == [False, 0], (n, p)
    assert cs["same_handles"]["a"] == cs["same_handles"]["b"] and cs["equal_gap_vs_bit"]["bit_keys"] == {"r0", "r1"}
    for p in PROCS:
        assert fx["all_rows_differ"][p]["count"] == fx["all_rows_differ"]["size"] == 2 * B + 500
        assert fx["first_at_row0"][p]["first"] == [True, 0]
        assert fx["first_at_last_row"][p]["first"] == [True, fx["first_at_last_row"]["size"] - 1]
        assert fx["first_in_last_of_40_columns"][p]["first"] == [True, 39 * B + 31337]
        assert fx["beyond_shorter_none"][p]["first"] == [False, 0]           # no size-difference term in the first mismatch
    assert fx["beyond_shorter_none"]["no_null"]["count"] == B + 300 - 700  # ... but one in the vector form
    assert fx["first_only_in_not_null"]["use_null"]["first"] == [True, B + 4242] and fx["first_only_in_not_null"]["no_null"]["first"] == [False, 0]
    assert fx["beyond_shorter_both"]["use_null"]["first"] == [True, B + 700] and fx["beyond_shorter_both"]["no_null"]["first"] == [False, 0]


@pytest.mark.parametrize("name", sorted(_fixture()["cases"]))
def test_port_replay_matches_reference_fixture(name, port):
    """the C port through the reference's own sequence (op2, set_range, find_first and nothing else)"""
    from sv_mismatch_cases import cases, oracle_case
    assert oracle_case(port, cases()[name]) == _fixture()["cases"][name]


@pytest.mark.parametrize("name", sorted(_fixture()["cases"]))
def test_value_model_matches_reference_fixture(name):
    """no planes and no oracle: a[i] != b[i] on the rows' values, then the size and NULL rules on unpacked bits"""
    from sv_mismatch_cases import cases, model_case
    assert model_case(cases()[name]) == _fixture()["cases"][name]


def test_generator_reproduces_fixture_where_the_reference_is_built():
    import oracle
    if not oracle.have_reference("avx2"):
        return                                               # (the committed fixture is what the other tests check)
    r = subprocess.run([sys.executable, os.path.join(GOLDEN, "make_sv_mismatch_golden.py"), "--check"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr


def test_entries_are_exported_and_refuse_a_null_context():
    """no GPU needed: the argument check comes before anything touches a device"""
    from bitmagic_amd import _ffi
    assert {"bmx_slice_mismatch", "bmx_slice_first_mismatch"} <= set(_ffi.exported_symbols())
    L = _ffi.lib()
    h, cnt, found, idx = C.c_void_p(), C.c_uint64(), C.c_int(), C.c_uint64()
    for proc in (0, 1):
        assert L.bmx_slice_mismatch(None, None, 0, 0, None, None, 0, 0, None, proc, C.byref(h), C.byref(cnt)) == _ffi.ERR_BADARG
        assert L.bmx_slice_first_mismatch(None, None, 0, 0, None, None, 0, 0, None, proc, C.byref(found), C.byref(idx)) == _ffi.ERR_BADARG
    assert h.value is None and b"ctx" in L.bmx_last_error()
    import bitmagic_amd as bm
    assert (bm.USE_NULL, bm.NO_NULL) == (0, 1)
    assert callable(bm.sparse_vector_find_mismatch) and callable(bm.sparse_vector_count_mismatch) and callable(bm.sparse_vector_find_first_mismatch)
