"""CPU: the batched range-count entries (bmx_slice_range_counts / _signed / bmx_gslice_range_counts) are exported, typed and refuse
a null context before any device call; the header cites the reference; the Python histogram wrapper builds the right closed
ranges (a stub stands in for the C call)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("bmx_slice_range_counts", "bmx_slice_range_counts_signed", "bmx_gslice_range_counts")


def test_entries_are_exported_and_typed():
    from bitmagic_amd import _ffi
    assert set(ENTRIES) <= set(_ffi.exported_symbols())
    L = _ffi.lib()
    for name in ENTRIES:
        fn = getattr(L, name)
        assert fn.restype is C.c_int and len(fn.argtypes) == 9 and fn.argtypes[5] is C.c_size_t and fn.argtypes[6] is C.c_uint64, name


def test_null_context_is_refused_without_a_device():
    from bitmagic_amd import _ffi
    L = _ffi.lib()
    lo, hi, out = np.array([1], np.uint64), np.array([2], np.uint64), np.full(1, 77, np.uint64)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    arr = (C.c_void_p * 1)()
    for name in ENTRIES:
        assert getattr(L, name)(None, arr, 0, p(lo), p(hi), 1, 65536, None, p(out)) == _ffi.ERR_BADARG, name
        assert getattr(L, name)(None, arr, 0, p(lo), p(hi), 0, 65536, None, p(out)) == _ffi.ERR_BADARG, name   # ... also with n == 0
    assert out[0] == 77


def test_header_cites_the_reference_and_agrees_with_the_binding():
    from bitmagic_amd import _ffi
    hdr = open(os.path.join(ROOT, "include", "bmx.h")).read()
    for name in ENTRIES:
        at = hdr.index("int %s(" % name)
        assert "src/bmsparsevec_algo.h:2862" in hdr[max(0, at - 2600):at], name
    m = re.search(r"#define BMX_RC_BATCH_MAX (\d+)", hdr)
    assert m and int(m.group(1)) == _ffi.RC_BATCH_MAX
    assert '"rc_batch"' in hdr and "rc_batch" in open(os.path.join(ROOT, "TUNING.md")).read()


class _Stub:
    """a scanner whose C call is replaced: records the closed ranges, answers hi - lo + 1 (one row per value; 0 for a reversed pair)"""

    def __init__(self, signed):
        import bitmagic_amd as bm
        self.s = object.__new__(bm.slice_scanner)
        self.s.slices, self.s.not_null, self.s._size, self.s.signed = [], None, 0, signed
        self.calls = []
        self.s._range_counts_call = self._call

    def _call(self, arr, lo, hi, out):
        assert lo.dtype == hi.dtype == (np.int64 if self.s.signed else np.uint64) and out.dtype == np.uint64
        self.calls.append((lo.tolist(), hi.tolist()))
        out[:] = [max(int(b) - int(a) + 1, 0) for a, b in zip(lo.tolist(), hi.tolist())]


def test_histogram_builds_closed_ranges():
    import bitmagic_amd as bm
    st = _Stub(False)
    got = st.s.histogram([0, 1, 1, 5, 16, 16, 16, 1 << 40, (1 << 64) - 1])
    assert st.calls == [([0, 1, 5, 16, 1 << 40], [0, 4, 15, (1 << 40) - 1, (1 << 64) - 2])]
    assert got.dtype == np.uint64 and got.tolist() == [1, 0, 4, 11, 0, 0, (1 << 40) - 16, (1 << 64) - 1 - (1 << 40)]
    st = _Stub(True)
    lo64, hi64 = -(1 << 63), (1 << 63) - 1
    got = st.s.histogram([lo64, -5, -5, 0, 7, hi64])
    assert st.calls == [([lo64, -5, 0, 7], [-6, -1, 6, hi64 - 1])]
    assert got.tolist() == [(1 << 63) - 5, 0, 5, 7, hi64 - 7]
    # nothing to count: no call at all
    st = _Stub(False)
    assert st.s.histogram([]).size == 0 and st.s.histogram([3]).size == 0 and st.s.histogram([3, 3]).tolist() == [0]
    assert st.s.find_range_counts([], []).size == 0 and st.calls == []
    # descending edges and bounds outside the container's type are refused before the call
    for signed, edges, status in ((False, [5, 3], bm._ffi.ERR_BADARG), (False, [-1, 3], bm._ffi.ERR_RANGE), (False, [0, 1 << 64], bm._ffi.ERR_RANGE),
                                  (True, [0, 1 << 63], bm._ffi.ERR_RANGE), (True, [-(1 << 63) - 1, 0], bm._ffi.ERR_RANGE)):
        st = _Stub(signed)
        with pytest.raises(bm.BmxError) as err:
            st.s.histogram(edges)
        assert err.value.status == status and st.calls == []
    st = _Stub(True)
    with pytest.raises(bm.BmxError) as err:
        st.s.find_range_counts([1, 2], [3])
    assert err.value.status == bm._ffi.ERR_BADARG
    assert st.s.find_range_counts([5, -3], [2, -3]).tolist() == [0, 1]               # (a reversed pair goes to the C entry as it is)
    assert st.calls == [([5, -3], [2, -3])]
