"""CPU: the cases and the model behind str_ref.json (string search over the planes of a bm::str_sparse_vector<>: find_eq_str and its
batch forms, src/bmsparsevec_algo.h:1194-1235, 2546-2588, 3263-3436): the model against plain loops, the shapes the GPU tests rely
on, the fixture against the reference where it is built, the Python group builder, the facade header alone, the declared entry."""
import ctypes as C
import json
import os
import re
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, GOLDEN)
REF = "/root/reference/src"
B = 65536


def _fx():
    with open(os.path.join(GOLDEN, "str_ref.json")) as f:
        return json.load(f)["cases"]


def test_fixture_is_small_and_covers_every_case():
    from bitmagic_amd import str_search_groups
    from str_cases import cases, model_case, record
    fx = _fx()
    assert os.path.getsize(os.path.join(GOLDEN, "str_ref.json")) < 100_000
    assert sorted(fx) == sorted(cases())
    for name, case in cases().items():
        assert dict(record(case, model_case(case), str_search_groups), anchored=fx[name]["anchored"]) == fx[name], name
        assert fx[name]["anchored"]["keys"] > 0 or fx[name]["n"] == 0 or name == "planes_0" or fx[name]["hits"] == 0, name


def test_model_against_a_plain_loop():
    from str_cases import cases, loop_case, model_case
    done = 0
    for name, case in cases().items():
        if case["size"] * case["keys"].shape[0] > 150_000:
            continue
        m, l = model_case(case), loop_case(case)
        assert np.array_equal(m["counts"], l["counts"]) and np.array_equal(m["first"], l["first"]), name
        assert np.array_equal(m["found"], l["counts"] > 0), name
        for q in range(case["keys"].shape[0]):                           # the row lists: ascending, as many as counted, first in front
            seg = m["ids"][int(m["offsets"][q]):int(m["offsets"][q + 1])]
            assert seg.size == m["counts"][q] and (np.diff(seg.astype(np.int64)) > 0).all() and (not seg.size or seg[0] == m["first"][q]), (name, q)
        done += 1
    assert done >= 10                                                    # the tails up to 2,049 rows and more


def test_case_shapes():
    """what the GPU tests rely on"""
    from str_cases import cases, key_strings, model_case
    cs, fx = cases(), _fx()
    g = cs["grid"]
    assert g["size"] == 14 * B + 1000 and len(g["planes"]) == 40 and g["planes"][13] is None and g["nn"] == "nn"
    assert (g["size"] + B - 1) // B - (g["vecs"]["p22"][1] + B - 1) // B == 2
    for p in (0, 1, 2, 3):                                               # a plane's columns cycle through the four block kinds
        held = np.bincount((g["vecs"]["p%d" % p][0] >> np.uint64(16)).astype(np.int64), minlength=15)
        assert {("null" if h == 0 else "full" if h == B else "some") for h in held[:14]} == {"null", "full", "some"}, p
    assert fx["grid"]["n_found"] >= fx["grid"]["n"] - 1 and b"" in key_strings(g)
    assert [len(cs["planes_%d" % P]["planes"]) for P in (0, 1, 8, 31, 32, 33, 64, 65, 72, 256, 257)] == [0, 1, 8, 31, 32, 33, 64, 65, 72, 256, 257]
    for P in (33, 64, 65, 72, 256, 257):                                 # keys that differ only in plane 31, only in plane 32
        k = cs["planes_%d" % P]["keys"].astype(np.int64)
        d = [tuple(np.flatnonzero(np.unpackbits((k[0] ^ k[q]).astype(np.uint8), bitorder="little"))) for q in range(1, k.shape[0])]
        assert (31,) in d and (32,) in d and (1,) in d and (P - 1,) in d, P
        m = model_case(cs["planes_%d" % P])
        assert (m["counts"][:4] > 1000).all(), P                         # each of them is spelled by many rows
    assert fx["planes_0"]["hits"] == 2 * B + 77 and fx["planes_0"]["n_found"] == 1      # no planes: the empty string is every row
    for size in (1, 31, 32, 33, 63, 64, 65, 2047, 2048, 2049, 65535, 65536, 65537):
        t = cs["tail_%d" % size]
        ids = t["vecs"]["p0"][0]                                         # plane 0: set in "yes" only
        inside, past = ids[ids < np.uint64(size)], ids[ids >= np.uint64(size)]
        assert past.size >= 4 and past[0] == size and (past >> np.uint64(16) == size >> 16).any() and (past >> np.uint64(16) > size >> 16).any()
        assert t["vecs"]["p0"][1] >= size + B
        assert model_case(t)["counts"][0] == inside.size >= 1
    assert [fx["keys_n%d" % n]["n"] for n in (0, 1, 2, 64, 65, 300, 3000)] == [0, 1, 2, 64, 65, 300, 3000]
    assert fx["keys_n3000"]["n_found"] == 3000 and fx["keys_n3000"]["hits"] > 100_000
    m = model_case(cs["keys_duplicates"])
    assert m["counts"][0] == m["counts"][2] == m["counts"][4] > 0 and m["counts"][3] == m["counts"][5] > 0
    e1, e0 = model_case(cs["keys_empty_with_nn"]), model_case(cs["keys_empty_without_nn"])
    assert 0 < e1["counts"][0] < e0["counts"][0] and e1["counts"][1] == e0["counts"][1] > 0
    assert list(model_case(cs["keys_absent_plane"])["counts"] > 0) == [False, True] and cs["keys_absent_plane"]["planes"][55] is None
    assert cs["keys_wider_zero_tail"]["keys"].shape[1] == 12 > 7 and (model_case(cs["keys_wider_zero_tail"])["counts"] > 0).all()
    assert list(model_case(cs["keys_wider_nonzero_tail"])["counts"] > 0) == [False, False, True]
    nm = model_case(cs["keys_narrower"])
    assert cs["keys_narrower"]["keys"].shape[1] == 3 and nm["counts"][0] == nm["counts"][2] == 1 and (nm["first"][0], nm["first"][2]) == (10, 11)   # "ab" is not "abc"
    d = cs["dictionary"]
    dm = model_case(d)
    assert d["size"] == 70000 == d["keys"].shape[0] and len(d["planes"]) == 128 and (dm["counts"] == 1).all()
    assert sorted(dm["first"].tolist()) == list(range(70000)) and dm["first"][0] != 0
    assert list(model_case(cs["every_row"])["counts"]) == [2 * B + 77, 0, 0]
    f = model_case(cs["first"])
    assert list(f["counts"]) == [2, 4, 0, 0] and list(f["first"]) == [13 * B + 9, 7000, 0, 0] and 7000 // 32 == 7003 // 32


def test_fixture_reproduces_from_the_reference():
    import oracle
    if not oracle.have_reference("avx2"):
        return                                                           # (the reference is built only where its sources are)
    r = subprocess.run([sys.executable, os.path.join(GOLDEN, "make_str_golden.py"), "--check"], capture_output=True, text=True)
    assert r.returncode == 0 and "reproduced" in r.stdout, r.stdout + r.stderr


def test_group_builder():
    """reverse octet order, the pre-screen, prefix_sub on and off (prepare_and_sub_aggregator, src/bmsparsevec_algo.h:2546-2588)"""
    from bitmagic_amd import str_search_groups
    from str_cases import cases, groups_of
    all24 = [True] * 24
    # "ab" = 0x61 0x62 over three octets: octet 1 first, AND ascending then SUB ascending per octet, then the planes above
    a, s = str_search_groups(b"ab", all24)
    assert a == [9, 13, 14, 0, 5, 6] and s == [8, 10, 11, 12, 15, 1, 2, 3, 4, 7] + list(range(16, 24))
    a2, s2 = str_search_groups(b"ab", all24, prefix_sub=False)
    assert a2 == a and s2 == [8, 10, 11, 12, 15, 1, 2, 3, 4, 7]
    assert str_search_groups(b"ab\0\0", all24) == (a, s)                 # padding is not part of the string
    holes = list(all24); holes[10] = False; holes[20] = False            # absent planes leave the SUB lists
    assert str_search_groups(b"ab", holes) == (a, [x for x in s if x not in (10, 20)])
    holes[13] = False                                                    # ... and a set bit without its plane: nothing matches
    assert str_search_groups(b"ab", holes) is None
    assert str_search_groups(b"abcd", all24) is None                     # longer than the column: a set bit beyond the planes
    assert str_search_groups(b"", all24) == ([], list(range(24))) and str_search_groups(b"", all24, False) == ([], [])
    assert str_search_groups(b"a", []) is None and str_search_groups(b"", []) == ([], [])
    fx = _fx()
    n = 0
    for name, case in cases().items():
        for prefix_sub, key in ((True, "groups"), (False, "groups_prefix")):
            assert groups_of(case, str_search_groups, prefix_sub) == fx[name][key], (name, key)
            n += len(fx[name][key])
    assert n > 100 and any(g[1] is None for c in fx.values() for g in c["groups"])


def test_scanner_builds_its_groups_in_one_place():
    """the Python facade without a device: remap tables, the C-string end, strings that cannot be spelled"""
    import bitmagic_amd as bm
    sc = object.__new__(bm.str_scanner)
    sc.planes, sc.not_null, sc._size, sc._rows, sc._longer, sc._remap = [object()] * 16, None, 10, None, False, None
    assert sc._code(b"ab\0cd") == b"ab"
    a, s = sc._group(b"a")
    assert len(a) == 3 and len(s) == 13
    t = np.zeros((2, 256), np.uint8)
    t[0, ord("a")], t[0, ord("b")], t[1, ord("a")] = 1, 2, 3
    sc.set_remap(t.tobytes(), 2)
    assert sc._code(b"aa") == b"\x01\x03" and sc._code(b"b") == b"\x02"
    assert sc._code(b"ab") is None and sc._code(b"aaa") is None and sc._group(b"ab") is None      # a character the position never holds; too long
    assert sc._code(b"") == b""
    sc.set_remap(None)
    assert sc._code(b"zz") == b"zz"


def test_entry_is_declared_and_refuses_null():
    from bitmagic_amd import _ffi
    assert "bmx_slice_eq_keys" in _ffi.exported_symbols()
    L = _ffi.lib()
    fn = L.bmx_slice_eq_keys
    assert fn.restype is C.c_int and len(fn.argtypes) == 11 and fn.argtypes[3] is C.c_uint64 and fn.argtypes[6] is C.c_size_t
    keys, out = np.array([[1, 2]], np.uint8), np.full(1, 77, np.uint64)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    arr = (C.c_void_p * 1)()
    assert fn(None, arr, 0, 65536, None, p(keys), 2, 1, p(out), None, None) == _ffi.ERR_BADARG
    assert fn(None, arr, 0, 65536, None, p(keys), 2, 0, p(out), None, None) == _ffi.ERR_BADARG           # ... also with n == 0
    assert out[0] == 77
    hdr = open(os.path.join(ROOT, "include", "bmx.h")).read()
    at = hdr.index("int bmx_slice_eq_keys(")
    for needle in ("src/bmsparsevec_algo.h:1194-1235", ":2546-2588", "src/bmstrsparsevec.h:1423", ":2569", ":2575-2586", ":3412-3415"):
        assert needle in hdr[at - 4000:at], needle
    m = re.search(r"#define BMX_EQK_MAX_PLANES (\d+)", hdr)
    assert m and int(m.group(1)) == _ffi.EQK_MAX_PLANES >= 1024
    tuning = open(os.path.join(ROOT, "TUNING.md")).read()
    for key in ("eqk_fp_bits", "eqk_pass_keys", "eqk_expand_kb"):
        assert '"%s"' % key in hdr and key in tuning, key


def test_kernel_holds_two_waves_per_simd_without_scratch():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import scratch_check
    ks = {k: v for k, v in scratch_check.kernels().items() if "k_slice_eq_keys" in k}
    assert len(ks) == 1
    for v in ks.values():
        assert v["scratch"] == 0 and v["vgpr"] <= 256                    # 512 threads per workgroup = two waves per SIMD


def test_facade_header_compiles_alone(tmp_path):
    """CPU: str_scanner.hpp needs nothing but the C header and the facade headers"""
    inc = os.path.join(ROOT, "include")
    a = tmp_path / "a.cpp"
    a.write_text('#include "bmx/str_scanner.hpp"\n'
                 'bool f(bmx::str_scanner& s, bmx::bvector& out, bmx::size_type& pos, const std::vector<std::string>& q,\n'
                 '       std::vector<uint64_t>& c, std::vector<bmx::size_type>& p, std::vector<uint8_t>& fd, const uint8_t* t)\n'
                 '{ s.set_remap(t, 4); s.find_eq_str_counts(q, c); s.find_eq_str_counts(q, c, true); s.find_eq_str_first(q, p, fd);\n'
                 '  s.find_eq_str_indices(q, c, p); s.find_eq_str_prefix("ab", out);\n'
                 '  return s.find_eq_str("ab", out) && s.find_eq_str("ab", pos); }\nint main(){return 0;}\n')
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I", inc, str(a)], check=True)


def test_adapter_overload_compiles_against_reference(tmp_path):
    """CPU, where the reference headers exist: the planes, the NULL vector and the remap matrix of a host bm::str_sparse_vector<>"""
    if not os.path.exists(os.path.join(REF, "bmstrsparsevec.h")):
        return                                                           # (nothing to compile against)
    src = tmp_path / "t.cpp"
    src.write_text('#include "bm.h"\n#include "bmstrsparsevec.h"\n#include "bmx/bm_adapter.hpp"\n'
                   'typedef bm::str_sparse_vector<char, bm::bvector<>, 32> str_sv_t;\n'
                   'void f(bmx::context& c, const str_sv_t& sv, bmx::str_scanner& sc, std::vector<bmx::bvector>& hold)\n'
                   '{ bmx::bind_str_scanner(c, sv, sc, hold); }\nint main(){return 0;}\n')
    subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-I", REF, "-I", os.path.join(ROOT, "include"), str(src)], check=True)
