"""The id lists of import_ref.json (bvector::set(ids, n, sort_order) on an empty vector, src/bm.h:4153) and the canonical form
of a block table that the fixture records.  Shared by make_import_golden.py and the tests; ids come from fixed seeds."""
from __future__ import annotations

import hashlib

import numpy as np

NULL, FULL, BIT, GAP = 0, 1, 2, 3
B = 65536


def _alternating(block: int, start: int, k: int) -> np.ndarray:
    """k isolated bits start, start + 2, ... of a block: 2k + 1 runs from an odd start, 2k from an even one"""
    return block * B + start + 2 * np.arange(k, dtype=np.uint64)


def _density(block: int, n: int, seed: int) -> np.ndarray:
    return block * B + np.sort(np.random.default_rng(seed).choice(B, size=n, replace=False)).astype(np.uint64)


# name -> (ids, nbits, reference flavour): flavour "avx2_64" for ids at or beyond 2^32 (the 48-bit address build)
def cases():
    c = {
        "empty_sized_from_ids": (np.zeros(0, np.uint64), 0, "avx2"),
        "empty_explicit_nbits": (np.zeros(0, np.uint64), 3 * B + 7, "avx2"),
        "id_0": (np.array([0], np.uint64), 0, "avx2"),
        "last_bit": (np.array([5 * B + 99], np.uint64), 5 * B + 100, "avx2"),
        "bits_65535_65536": (np.array([65535, 65536], np.uint64), 0, "avx2"),
        "duplicates": (np.array([7, 7, 7, 100000, 7, 100000, 3, 65535, 3], np.uint64), 0, "avx2"),
        "full_block": (np.concatenate([np.array([17], np.uint64), B + np.arange(B, dtype=np.uint64)]), 0, "avx2"),
        "runs_1275": (_alternating(1, 1, 637), 0, "avx2"),
        "runs_1276": (_alternating(1, 0, 638), 0, "avx2"),
        "density_10pct": (_density(2, 6554, 11), 0, "avx2"),
        "trailing_null_blocks": (np.array([1, 2, 3, 40000], np.uint64), 10 * B + 5, "avx2"),
        "mixed_blocks": (np.concatenate([np.array([0, 1, 2, 999], np.uint64), _density(1, 655, 12), 3 * B + np.arange(B, dtype=np.uint64),
                                         _density(4, 20000, 13), _alternating(6, 1, 637), _alternating(7, 0, 638),
                                         np.array([9 * B + 65535], np.uint64)]), 9 * B + 300, "avx2"),
        "ids_beyond_2_32": (np.array([(1 << 32) + 5, (1 << 33) + 3 * B + 1, 5 * (1 << 32) + 77, 5], np.uint64), 0, "avx2_64"),
        "dense_beyond_2_32": (np.concatenate([(1 << 32) - 2 * B + _density(0, 3000, 14), (1 << 32) + np.arange(B, dtype=np.uint64),
                                              (1 << 34) + _density(0, 30000, 15)]), (1 << 34) + 7 * B, "avx2_64"),
    }
    return c


def sha(a: np.ndarray) -> str:
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def canonical(kinds, offs, bit_slab, gap_slab):
    """a flattened block table in the layout the device writes (k_emit_blocks): bit-blocks by ordinal, GAP blocks from 16-byte
    boundaries (offsets in words, multiples of 8) padded with 0xFFFF, level bits masked (an allocator detail)
    -> (kinds, offs, bit_slab, gap_slab)"""
    kinds = np.asarray(kinds, np.uint8); offs = np.asarray(offs, np.uint32)
    gap_slab = np.asarray(gap_slab, np.uint16)
    out_offs = offs.copy()
    parts, pos = [], 0
    for nb in np.nonzero(kinds == GAP)[0]:
        o = int(offs[nb]); n = (int(gap_slab[o]) >> 3) + 1
        g = np.full((n + 7) & ~7, 0xFFFF, np.uint16)
        g[:n] = gap_slab[o:o + n]
        g[0] &= 0xFFF9
        parts.append(g); out_offs[nb] = pos; pos += g.size
    gaps = np.concatenate(parts) if parts else np.zeros(0, np.uint16)
    return kinds, out_offs, np.asarray(bit_slab, np.uint32), gaps


def record(kinds, offs, bit_slab, gap_slab) -> dict:
    k, o, b, g = canonical(kinds, offs, bit_slab, gap_slab)
    return {"nblocks": int(k.size), "counts": [int((k == i).sum()) for i in range(4)], "kinds_sha": sha(k), "offs_sha": sha(o),
            "bit_sha": sha(b), "gap_sha": sha(g), "gap_words": int(g.size)}


def oracle_table(o, ids, nbits: int, optimize: bool):
    """bvector::set(ids) as the oracle / reference API does it: set_bit per id on a vector of nbits' bits, optimize() when asked
    -> (nbits', flattened table).  A default bm::bvector<> allocates the bit-blocks the bulk set(ids, n, so) allocates."""
    nbits_out = max(int(nbits), int(ids.max()) + 1 if ids.size else 0)
    v = o.new(nbits_out)
    for p in ids:
        v.set_bit(int(p))
    if optimize:
        v.optimize()
    v.nbits = nbits_out
    return nbits_out, v.flatten(), v.count()
