"""CPU: the C-ABI library loads and exports every symbol include/bmx.h declares
(no compute calls without a GPU), and the host-side mirror keeps the reference's
argument / error behaviour."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_every_declared_symbol():
    from bitmagic_amd import _ffi
    names = _ffi.exported_symbols()
    assert len(names) >= 30
    L = C.CDLL(_ffi.LIB_PATH)
    missing = [n for n in names if not hasattr(L, n)]
    assert not missing, missing
    L2 = _ffi.lib()                       # typed loader must also accept the library
    assert L2.bmx_simd_version() == 950
    assert b"BMX-00" in L2.bmx_error_msg(0) and b"BMX-03" in L2.bmx_error_msg(3)


def test_header_cites_reference_for_each_entry_point():
    txt = open(os.path.join(ROOT, "include", "bmx.h")).read()
    assert 'extern "C"' in txt
    assert "torch" not in txt.lower()
    for ref in ("src/bm.h:6185", "src/bmaggregator.h:1162", "src/bmaggregator.h:1292", "src/bm.h:2531",
                "src/bm.h:5350", "src/bmalgo.h:49", "src/bmbvimport.h:46", "libbm.h"):
        assert ref in txt, ref


def test_product_never_touches_oracle():
    """the shipped package must not import / load anything under oracle/"""
    pkg = os.path.join(ROOT, "bitmagic_amd")
    for dp, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".h", ".hip", ".hpp", ".cpp")):
                src = open(os.path.join(dp, f)).read()
                assert not re.search(r"^\s*(import|from)\s+oracle", src, re.M), f
                assert "libbmx_oracle" not in src and "libbmref" not in src, f


def test_arg_groups_semantics():
    """arg_groups::add: group index > 1 is BM_ERR_RANGE, nullptr is ignored
    (src/bmaggregator.h:2931-2947)"""
    import bitmagic_amd as bm
    ag = bm.arg_groups()
    assert ag.add(None, 0) == 0 and ag.arg_bv0 == []
    with pytest.raises(bm.BmxError) as e:
        ag.add(None, 2)
    assert e.value.status == 3


def test_no_device_fails_loudly():
    """on a machine without a GPU the context must raise, never fall back"""
    import bitmagic_amd as bm
    try:
        import torch
        has_gpu = torch.cuda.is_available()
    except Exception:
        has_gpu = False
    if has_gpu:
        pytest.skip("GPU present")
    with pytest.raises(bm.BmxError):
        bm.context(0)


def test_slice_scanner_group_rule():
    """prepare_and_sub_aggregator (src/bmsparsevec_algo.h:2593-2640) as mirrored by slice_scanner: AND group =
    planes of the set bits, high bit first; SUB group = every other existing plane; a set bit without a plane
    (absent or beyond effective_slices) means nothing can match; value 0 has no AND group (it goes through the comparison kernel)"""
    import bitmagic_amd as bm

    class fake_ctx:            # group construction is host logic: no device call
        _h = None
    planes = ["p0", "p1", None, "p3", "p4"]            # plane 2 does not exist
    sc = bm.slice_scanner(fake_ctx(), planes)
    assert sc._groups(0b11011) == (["p4", "p3", "p1", "p0"], [])
    assert sc._groups(0b01001) == (["p3", "p0"], ["p1", "p4"])
    assert sc._groups(0b00100) is None                  # needs the absent plane
    assert sc._groups(1 << 5) is None                   # bit above every plane
    with pytest.raises(bm.BmxError) as e:
        sc._groups(0)
    assert e.value.status == 2


def test_shard_ranges_cover_every_block_once():
    from bitmagic_amd import shard_range
    for nblocks in (0, 1, 7, 15259, 61036):
        for world in (1, 2, 3, 8):
            r = [shard_range(nblocks, k, world) for k in range(world)]
            assert r[0][0] == 0 and r[-1][1] == nblocks
            assert all(a[1] == b[0] for a, b in zip(r, r[1:]))
            sizes = [hi - lo for lo, hi in r]
            assert max(sizes) - min(sizes) <= 1


def test_bench_refuses_more_gpus_than_visible():
    """`python bench.py --gpus 8` without a launcher must use 8 devices or exit non-zero -- never print a 1-GPU line
    (VERDICT r2 item 1).  On this CPU box no device is visible, so both in-process and torchrun-style starts must fail."""
    import subprocess
    import sys
    import torch
    if torch.cuda.device_count() >= 8:
        pytest.skip("8 devices visible: nothing to refuse")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT", "BMX_BENCH_TEST_ONE_DEVICE")}
    out = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "8", "--no-cpu", "--steps", "1", "--warmup", "0"],
                         env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode != 0
    assert not any(l.startswith("{") for l in out.stdout.splitlines())
    assert "needs 8 visible devices" in out.stderr
    # a launcher that started fewer ranks than --gpus asks for is refused as well
    env2 = dict(env, RANK="0", WORLD_SIZE="1", LOCAL_RANK="0", MASTER_PORT="29999", MASTER_ADDR="127.0.0.1")
    out = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "8", "--no-cpu", "--steps", "1", "--warmup", "0"],
                         env=env2, capture_output=True, text=True, timeout=300)
    assert out.returncode != 0 and not any(l.startswith("{") for l in out.stdout.splitlines())


def test_traffic_figures_are_stamped_and_dropped_on_mismatch(tmp_path, monkeypatch):
    """roofline.traffic comes from PMC passes of a separate rocprofv3 run (profiles/traffic_*.json): every committed file carries
    the kernel and the commit it was measured on, and bench.py drops a figure -- traffic None, the reason in traffic_source --
    when the stamp is missing or names another kernel than the one the run reports"""
    import json
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if root not in sys.path: sys.path.insert(0, root)
    import bench
    import glob
    files = sorted(glob.glob(os.path.join(root, "profiles", "traffic_*.json")))
    assert len(files) >= 6
    for f in files:
        j = json.load(open(f))
        assert j.get("kernel") and j.get("commit") and j.get("hbm_bytes_per_launch", 0) > 0 and j.get("workload"), f
    # the live loader: right kernel -> the figure; another kernel -> dropped with a reason; workload filter
    t, src, _ = bench.traffic_file("traffic_config4.json", kernel="k_agg_or_rows<4>: tiles of 14 block columns")
    assert t and "k_agg_or_rows" in src and "commit" in src
    t, src, _ = bench.traffic_file("traffic_config4.json", kernel="k_agg_or_gap_tiled<1,1> (descriptor-table kernel)")
    assert t is None and src.startswith("dropped")
    t, src, _ = bench.traffic_file("traffic_latest.json", kernel="k_pipe_counts_bits2<4,true,640,8> x 6 launches", workload="agg_and_count_64x1000000000")
    assert t is None and src is None                          # another workload: no figure, nothing to explain
    # an unstamped file is refused
    monkeypatch.setattr(bench, "ROOT", str(tmp_path))
    os.makedirs(tmp_path / "profiles")
    json.dump({"workload": "w", "hbm_bytes_per_launch": 1, "source": "s"}, open(tmp_path / "profiles" / "traffic_x.json", "w"))
    t, src, _ = bench.traffic_file("traffic_x.json", kernel="k")
    assert t is None and "not stamped" in src


def test_no_kernel_of_the_default_build_touches_scratch():
    """register spills on default paths (k_agg_and_sub<4,640> 80 B / lane, k_pipe_counts_bits2<4,false,640,8>
    116 B, k_slice_eq_counts_big<32,...,8> 12 B).  The AMDGPU notes of the gfx950 code object inside libbmx.so list the
    private segment (scratch) and the VGPR spill count of every kernel: both must be zero (tools/scratch_check.py; no GPU needed)."""
    import importlib.util
    import shutil
    spec = importlib.util.spec_from_file_location("scratch_check", os.path.join(ROOT, "tools", "scratch_check.py"))
    sc = importlib.util.module_from_spec(spec); spec.loader.exec_module(sc)
    if not os.path.exists(sc.READELF):
        pytest.skip("llvm-readelf of the ROCm toolchain not found")
    ks = sc.kernels()
    assert len(ks) > 150, "the code object's kernel records were not found"
    # (SGPR spills go to VGPR lanes, not to memory: they are not scratch)
    bad = {k: v for k, v in ks.items() if v["scratch"] or v["vgpr_spill"]}
    assert not bad, bad


def test_no_exception_crosses_the_abi():
    """lang-maps/libbm/src/libbm.cpp:28-35: every body of the reference's C wrapper is a try / catch that turns std::bad_alloc into
    BM_ERR_BADALLOC -- a C caller never sees a C++ exception.  Every extern "C" body of libbmx.so sits in the same barrier
    (ABI_TRY / ABI_END); bmx_debug_inject_failure makes the next entry throw at its first statement: what comes back must be a
    status, and the library must work afterwards.  (No GPU needed: the throw precedes any device call.)"""
    from bitmagic_amd import _ffi
    L = _ffi.lib()
    null = C.c_void_p()
    out = C.c_void_p()
    def upload():                                       # a call that is BADARG on any machine (null context)
        return L.bmx_vec_upload(null, 0, 0, None, None, None, 0, None, 0, C.byref(out))
    assert upload() == _ffi.ERR_BADARG
    for kind, status, text in ((1, _ffi.ERR_BADALLOC, b"bad_alloc"), (2, _ffi.ERR_DEVICE, b"length_error"), (3, _ffi.ERR_DEVICE, b"not a std::exception")):
        assert L.bmx_debug_inject_failure(null, kind, 0) == 0
        assert upload() == status and text in L.bmx_last_error(), (kind, L.bmx_last_error())
        assert upload() == _ffi.ERR_BADARG              # one shot: the library goes on
    # `after` counts entries: two calls pass, the third throws -- through another entry point (the group layer's barrier)
    assert L.bmx_debug_inject_failure(null, 1, 2) == 0
    assert upload() == _ffi.ERR_BADARG and upload() == _ffi.ERR_BADARG
    n = C.c_int32()
    assert L.bmx_group_size(null, C.byref(n)) == _ffi.ERR_BADALLOC
    assert L.bmx_group_size(null, C.byref(n)) == _ffi.ERR_BADARG
    # disarm
    assert L.bmx_debug_inject_failure(null, 1, 5) == 0 and L.bmx_debug_inject_failure(null, 0, 0) == 0
    for _ in range(8): assert upload() == _ffi.ERR_BADARG


def test_injection_counts_only_the_callers_entries():
    """`after` counts the entries the caller makes: an entry point that calls another one (bmx_vec_generate ->
    bmx_vec_generate_shard) takes one step, and bmx_debug_inject_failure itself takes none -- disarming an injection that is due at
    the next entry returns OK and leaves nothing armed"""
    from bitmagic_amd import _ffi
    L = _ffi.lib()
    null = C.c_void_p()
    out = C.c_void_p()
    def generate():                                     # BADARG on any machine (null context), through the nested entry
        return L.bmx_vec_generate(null, 1, 0, 0, 655, 65536, 0, C.byref(out))
    assert L.bmx_debug_inject_failure(null, 1, 1) == 0
    assert generate() == _ffi.ERR_BADARG                # one step, not two
    assert generate() == _ffi.ERR_BADALLOC and b"bad_alloc" in L.bmx_last_error()
    assert generate() == _ffi.ERR_BADARG
    assert L.bmx_debug_inject_failure(null, 1, 0) == 0
    assert L.bmx_debug_inject_failure(null, 0, 0) == 0  # the disarm is not the entry that throws
    assert generate() == _ffi.ERR_BADARG
    n = C.c_int32()
    assert L.bmx_group_size(null, C.byref(n)) == _ffi.ERR_BADARG
    # kind 6 arms the device-allocation countdown of a context: it needs one
    assert L.bmx_debug_inject_failure(null, 6, 0) == _ffi.ERR_BADARG


def test_every_abi_body_sits_in_the_barrier():
    """each `int bmx_*` that include/bmx.h declares is defined with ABI_TRY ... ABI_END in bmx.hip / bmx_group.hip"""
    hdr = open(os.path.join(ROOT, "include", "bmx.h")).read()
    names = set(re.findall(r"^int\s+(bmx_\w+)\s*\(", hdr, re.M))
    src = "".join(open(os.path.join(ROOT, "bitmagic_amd", "csrc", f)).read() for f in ("bmx.hip", "bmx_group.hip"))
    missing = []
    for n in sorted(names):
        m = re.search(r"^int\s+%s\s*\([^{;]*\)\s*\{([^\n]*)" % n, src, re.M | re.S)
        assert m, n
        if "ABI_TRY" not in m.group(1) and n != "bmx_simd_version": missing.append(n)
    assert not missing, missing
