"""String search over the device-resident planes of a bm::str_sparse_vector<>: the find_eq_str half of
bm::sparse_vector_scanner (src/bmsparsevec_algo.h:1194-1235, 3263-3436).  Plane octet * 8 + bit holds bit `bit` of character
`octet` of every row (src/bmstrsparsevec.h:1423).

Not here: bfind_eq_str / lower_bound_str (binary search over a sorted vector) and rank-select-compressed string vectors (the
reference does not search those either, :3382-3386)."""
from __future__ import annotations

import ctypes as C
from typing import Sequence

import numpy as np

from . import _ffi
from ._ffi import BmxError, check, lib

# batches of at least this many strings take the one-pass batch entry (bmx_slice_eq_keys) instead of one AND-SUB group per
# string (TUNING.md "str_scanner": the measured crossover)
BATCH_MIN = 64


def str_search_groups(key: bytes, present: Sequence[bool], prefix_sub: bool = True):
    """The AND-SUB group of one (remapped) string as plane numbers -> (and_planes, sub_planes), or None when the string has a bit
    no plane holds (prepare_and_sub_aggregator, src/bmsparsevec_algo.h:2546-2588).  key: the characters up to the first zero;
    present[p]: plane p exists.  Octets go in reverse order (:2559); per octet the set bits ascending into AND, then the clear
    bits whose plane exists ascending into SUB (add_agg_char, :1817-1853); with prefix_sub every existing plane from
    8 * len(key) upward goes into SUB (:2575-2586).  A pure function of its arguments.  (Trailing zero octets are padding; a
    zero octet inside the key -- nothing a C string can hold -- takes part like any other: no AND plane, its planes into SUB.)"""
    key = bytes(key).rstrip(b"\0")
    nplanes = len(present)
    a, s = [], []
    for octet in range(len(key) - 1, -1, -1):
        value = key[octet]
        mask = 0
        for b in range(8):
            p = octet * 8 + b
            if p < nplanes and present[p]:
                mask |= 1 << b
        if value & mask != value:                                   # pre-screen for impossible values (:2569)
            return None
        a.extend(octet * 8 + b for b in range(8) if (value >> b) & 1)
        s.extend(octet * 8 + b for b in range(8) if ((value ^ 0xFF) & mask) >> b & 1)
    if prefix_sub:
        s.extend(p for p in range(len(key) * 8, nplanes) if present[p])
    return a, s


class str_scanner:
    """bm::sparse_vector_scanner<bm::str_sparse_vector<..>> over resident planes.  planes[p] = device vector of plane p (None =
    the plane does not exist), size = sv.size(), not_null = sv.get_null_bvector() or None."""

    def __init__(self, ctx, planes=(), size: int | None = None, not_null=None):
        from . import aggregator
        self.ctx = ctx
        self.agg = aggregator(ctx)
        self._remap = None
        self.bind(planes, size, not_null)

    def bind(self, planes, size: int | None = None, not_null=None):
        self.planes = list(planes)
        self.not_null = not_null
        self._size = size
        self._rows = None
        self._longer = None
        return self

    def size(self) -> int:
        if self._size is None:
            self._size = max([p.size() for p in self.planes if p is not None], default=0)
        return self._size

    def set_remap(self, tables, octets: int | None = None):
        """one 256-entry code table per octet position (str_sparse_vector::get_remap_matrix(): remap_matrix2_); a character mapped
        to 0 is in no row at that position: the string is not found (remap_tosv returning false, :3394-3396).  None: no remap."""
        if tables is None:
            self._remap = None
            return self
        t = np.frombuffer(tables, np.uint8) if isinstance(tables, (bytes, bytearray)) else np.ascontiguousarray(tables, np.uint8)
        self._remap = t.reshape(-1, 256) if octets is None else t.reshape(octets, 256)
        return self

    # ---- one string -> its code, its group ----
    def _code(self, s: bytes):
        """the characters the planes hold for s (None: not representable, nothing matches)"""
        s = bytes(s)
        z = s.find(b"\0")
        if z >= 0:
            s = s[:z]
        if self._remap is None:
            return s
        if len(s) > self._remap.shape[0]:
            return None
        out = bytes(int(self._remap[i, ch]) for i, ch in enumerate(s))
        return None if 0 in out else out

    def _present(self):
        return [p is not None for p in self.planes]

    def _row_set(self):
        """AND operands that bound every search to the rows: [0, size) and the not-NULL vector (the empty string only)"""
        if self._rows is None:
            from . import bvector
            n = self.size()
            self._rows = bvector.from_ranges(self.ctx, np.array([[0, n - 1]], np.uint64), n) if n else None
        return ([self._rows] if self._rows is not None else []) + ([self.not_null] if self.not_null is not None else [])

    def _group(self, s: bytes, prefix_sub: bool = True):
        """-> (AND vectors, SUB vectors) or None (nothing can match).  All searches build their groups here."""
        code = self._code(s)
        if code is None:
            return None
        if not code:                                                 # the empty string: find_zero with null correction (:3412-3415)
            if not self.size():
                return None
            return self._row_set(), [p for p in self.planes if p is not None]
        g = str_search_groups(code, self._present(), prefix_sub)
        if g is None or not self.size():
            return None
        if self._longer is None:                                     # planes that run past size: the column's rows join the AND list
            self._longer = any(p is not None and p.size() > self.size() for p in self.planes)
        return [self.planes[p] for p in g[0]] + (self._row_set()[:1] if self._longer else []), [self.planes[p] for p in g[1]]

    # ---- single searches ----
    def find_eq_str(self, s: bytes):
        """find_eq_str(sv, str, bv_out) :1194 -> (bv_out or None, found)"""
        g = self._group(s, True)
        if g is None:
            return None, False
        return self.agg.combine_and_sub(g[0], g[1])

    def find_eq_str_prefix(self, s: bytes):
        """find_eq_str_prefix :1221: rows that START with s -> (bv_out or None, found)"""
        if self._code(s) == b"":                                     # the empty prefix: every row
            return self.agg.combine_and_sub(self._row_set()[:1], []) if self.size() else (None, False)
        g = self._group(s, False)
        if g is None:
            return None, False
        return self.agg.combine_and_sub(g[0], g[1])

    def find_first_eq_str(self, s: bytes):
        """find_eq_str(sv, str, pos) :1208 -> (found, pos): the lowest matching row"""
        g = self._group(s, True)
        if g is None:
            return False, 0
        return self.agg.find_first_and_sub(g[0], g[1])

    # ---- batches ----
    def _use_batch(self, n: int, use_pipeline) -> bool:
        if use_pipeline is None:
            use_pipeline = False
        if use_pipeline or len(self.planes) > _ffi.EQK_MAX_PLANES:
            return False
        return n >= BATCH_MIN

    def _eq_keys(self, strs, want_counts: bool, want_first: bool):
        codes = [self._code(s) for s in strs]
        n = len(codes)
        kb = max([len(c) for c in codes if c is not None], default=0)
        kb = max(kb, (len(self.planes) + 7) // 8, 1) + 1             # one octet more than the column: an unrepresentable string's mark
        keys = np.zeros((n, kb), np.uint8)
        for q, c in enumerate(codes):
            if c is None:
                keys[q, kb - 1] = 1                                  # a bit no plane holds: matches nothing
            elif c:
                keys[q, :len(c)] = np.frombuffer(c, np.uint8)
        return self.eq_keys(keys, want_counts, want_first)

    def eq_keys(self, keys, want_counts: bool = True, want_first: bool = True):
        """bmx_slice_eq_keys as it is: keys = an (n, key_bytes) uint8 array, bit b of octet j = plane 8 j + b, no remap, always the
        batch kernel -> (counts or None, first or None, found or None)"""
        keys = np.ascontiguousarray(keys, np.uint8)
        if keys.ndim != 2:
            raise BmxError(_ffi.ERR_BADARG, "Invalid argument", "keys: an (n, key_bytes) array expected")
        n, kb = keys.shape
        if kb == 0:
            keys, kb = np.zeros((n, 1), np.uint8), 1
        counts =np.zeros(n, np.uint64) if want_counts else None
        first = np.zeros(n, np.uint64) if want_first else None
        found = np.zeros(n, np.uint8) if want_first else None
        arr = (C.c_void_p * max(len(self.planes), 1))()
        for i, p in enumerate(self.planes):
            arr[i] = p._h if p is not None else None
        vp = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None
        check(lib().bmx_slice_eq_keys(self.ctx._h, arr, len(self.planes), self.size(),
                                      self.not_null._h if self.not_null is not None else None,
                                      vp(keys), kb, n, vp(counts), vp(first), vp(found)))
        return counts, first, found

    def _pipeline(self, strs, opt):
        from . import pipeline
        pipe = pipeline(self.ctx, opt)
        slot = []
        for s in strs:
            g = self._group(s, True)
            if g is None:
                slot.append(-1); continue
            ag = pipe.add()
            for x in g[0]: ag.add(x, 0)
            for x in g[1]: ag.add(x, 1)
            slot.append(pipe.size() - 1)
        if pipe.size():
            pipe.complete()
        return pipe, slot

    def find_eq_str_counts(self, strs, use_pipeline: bool | None = None) -> np.ndarray:
        """counts[q] = rows equal to strs[q]: the batch entry (one pass over the planes for the whole batch), or one counts
        pipeline with a group per string -- the reference's find_eq_str(pipe), :3263.  Default: the batch entry from BATCH_MIN
        strings upward."""
        strs = list(strs)
        if not strs:
            return np.zeros(0, np.uint64)
        if self._use_batch(len(strs), use_pipeline):
            return self._eq_keys(strs, True, False)[0]
        from . import agg_opt_only_counts
        pipe, slot = self._pipeline(strs, agg_opt_only_counts)
        out = np.zeros(len(strs), np.uint64)
        if pipe.size():
            cnt = self.agg.combine_and_sub(pipe)
            for q, sl in enumerate(slot):
                if sl >= 0: out[q] = cnt[sl]
        return out

    def find_eq_str_first(self, strs, use_pipeline: bool | None = None):
        """-> (pos, found): the lowest row equal to strs[q] (pos 0 where not found)"""
        strs = list(strs)
        if not strs:
            return np.zeros(0, np.uint64), np.zeros(0, bool)
        if self._use_batch(len(strs), use_pipeline):
            _, first, found = self._eq_keys(strs, False, True)
            return first, found.astype(bool)
        pos, found = np.zeros(len(strs), np.uint64), np.zeros(len(strs), bool)
        for q, s in enumerate(strs):
            g = self._group(s, True)
            if g is not None:
                f, p = self.agg.find_first_and_sub(g[0], g[1])
                found[q], pos[q] = f, p if f else 0
        return pos, found

    def find_eq_str_indices(self, strs):
        """-> (offsets, ids): ids[offsets[q]:offsets[q + 1]] = the rows equal to strs[q], ascending -- one index-list pipeline
        run for the batch (aggregator.combine_and_sub_indices), as slice_scanner.find_eq_indices"""
        from . import agg_opt_disable_bvects_and_counts
        strs = list(strs)
        pipe, slot = self._pipeline(strs, agg_opt_disable_bvects_and_counts)
        poff, pids = np.zeros(1, np.uint64), np.zeros(0, np.uint64)
        if pipe.size():
            poff, pids = self.agg.combine_and_sub_indices(pipe)
        if pipe.size() == len(strs):
            return poff, pids
        empty = np.zeros(0, np.uint64)
        parts = [pids[int(poff[s]):int(poff[s + 1])] if s >= 0 else empty for s in slot]
        offsets = np.zeros(len(strs) + 1, np.uint64)
        offsets[1:] = np.cumsum([p.size for p in parts], dtype=np.uint64)
        return offsets, (np.concatenate(parts) if parts else empty)
