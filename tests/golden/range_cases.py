"""The pair lists of range_ref.json (bvector::set_range(l, r) for every pair on an empty vector, then optimize(); src/bm.h:2398) and
the interval form of a vector (what a bm::interval_enumerator loop yields, src/bmintervals.h:52-226).  Shared by
make_range_golden.py and the tests; pairs come from fixed seeds.  The canonical form of a block table is import_cases.record()."""
from __future__ import annotations

import numpy as np

from import_cases import record, sha  # noqa: F401

B = 65536


def _pairs(*p) -> np.ndarray:
    return np.array(p, np.uint64).reshape(-1, 2)


def _singles(block: int, start: int, k: int) -> np.ndarray:
    """k isolated bits start, start + 2, ... of a block as one-bit intervals: 2k + 1 runs from an odd start, 2k from an even one"""
    p = block * B + start + 2 * np.arange(k, dtype=np.uint64)
    return np.stack([p, p], axis=1)


def _random_pairs(seed: int, n: int, nblocks: int, max_len: int) -> np.ndarray:
    rng = np.random.default_rng(seed)
    l = rng.integers(0, nblocks * B - max_len, size=n).astype(np.uint64)
    r = l + rng.integers(0, max_len, size=n).astype(np.uint64)
    p = np.stack([l, r], axis=1)
    rng.shuffle(p, axis=0)
    return p


def _every7(nblocks: int) -> np.ndarray:
    l = np.arange(0, nblocks * B - 2, 7, dtype=np.uint64)
    return np.stack([l, l + 2], axis=1)


# name -> (pairs (n, 2) uint64, nbits, reference flavour): flavour "avx2_64" for ends at or beyond 2^32
def cases():
    return {
        "empty": (np.zeros((0, 2), np.uint64), 3 * B + 7, "avx2"),
        "bit_0": (_pairs(0, 0), 0, "avx2"),
        "swapped": (_pairs(70000, 10), 0, "avx2"),
        "across_border": (_pairs(65535, 65536), 0, "avx2"),
        "exactly_block_1": (_pairs(B, 2 * B - 1), 0, "avx2"),
        "ends_at_65535": (_pairs(500, B - 1, B + 300, 3 * B - 1), 0, "avx2"),
        "long_span": (_pairs(12345, 40 * B + 17), 50 * B, "avx2"),
        "touching": (_pairs(10, 19, 20, 29, 30, 30, 65535, 65535, 65536, 65536), 0, "avx2"),
        "overlap_nested_dup": (_pairs(300, 3 * B + 50, 2 * B, 3 * B + 10, 3 * B + 40, 6 * B + 500, 300, 3 * B + 50, 100, 200, 150, 200),
                               0, "avx2"),
        "runs_1275": (_singles(1, 1, 637), 0, "avx2"),
        "runs_1276": (_singles(1, 0, 638), 0, "avx2"),
        "union_is_block_2": (_pairs(2 * B + 30000, 3 * B - 1, 2 * B, 2 * B + 40000), 0, "avx2"),
        "random_4000": (_random_pairs(21, 4000, 20, 400), 0, "avx2"),
        "beyond_2_32": (_pairs((1 << 32) - 10, (1 << 32) + B + 5, (1 << 33) + 3, (1 << 33) - B - 7, 1 << 32, (1 << 32) + 100), 0, "avx2_64"),
        "every_7_bits": (_every7(4), 0, "avx2"),
    }


def orders(pairs: np.ndarray):
    """the same set of pairs in the orders the device must not tell apart: name -> (n, 2) array"""
    out = {"given": pairs, "sorted": pairs[np.argsort(pairs.min(axis=1), kind="stable")] if len(pairs) else pairs,
           "reversed": pairs[::-1], "ends_swapped": pairs[:, ::-1]}
    for seed in (1, 2):
        out[f"shuffled{seed}"] = pairs[np.random.default_rng(seed).permutation(len(pairs))]
    return {k: np.ascontiguousarray(v) for k, v in out.items()}


def runs_of_words(words: np.ndarray) -> np.ndarray:
    """the maximal runs of ones of a vector given as 32-bit words -> (n, 2) uint64 of inclusive [left, right], ascending.
    A start is a one whose predecessor is zero, an end a one whose successor is zero; words are walked in slices so that a
    vector of 2^33 bits needs no array of its bits."""
    words = np.ascontiguousarray(words, np.uint32)
    starts, ends = [], []
    step = 1 << 22
    for w0 in range(0, words.size, step):
        x = words[w0:w0 + step]
        if not x.any():
            continue
        prev = np.empty_like(x); prev[1:] = x[:-1] >> 31; prev[0] = (words[w0 - 1] >> 31) if w0 else 0
        nxt = np.empty_like(x); nxt[:-1] = x[1:] & 1; nxt[-1] = (words[w0 + x.size] & 1) if w0 + x.size < words.size else 0
        for mask, dst in ((x & ~((x << 1) | prev), starts), (x & ~((x >> 1) | (nxt << 31)), ends)):
            nz = np.flatnonzero(mask)
            bits = np.unpackbits(mask[nz].view(np.uint8).reshape(-1, 4), axis=1, bitorder="little")
            wi, bi = np.nonzero(bits)
            dst.append((w0 + nz[wi]).astype(np.uint64) * 32 + bi.astype(np.uint64))
    s = np.concatenate(starts) if starts else np.zeros(0, np.uint64)
    e = np.concatenate(ends) if ends else np.zeros(0, np.uint64)
    assert s.size == e.size
    return np.stack([s, e], axis=1)


def oracle_table(o, pairs: np.ndarray, nbits: int):
    """set_range per pair on a vector of nbits' bits, optimize(), as the oracle / reference API does it
    -> (nbits', flattened table, count, intervals (n, 2) from the vector's own words)"""
    nbits_out = max(int(nbits), int(pairs.max()) + 1 if pairs.size else 0)
    v = o.new(nbits_out)
    for l, r in pairs:
        l, r = int(l), int(r)
        if not o.is_ref:                                   # the reference swaps right < left itself (src/bm.h:2407)
            l, r = min(l, r), max(l, r)
        v.set_range(l, r)
    v.optimize()
    v.nbits = nbits_out
    nblocks = (nbits_out + B - 1) // B
    return nbits_out, v.flatten(), v.count(), runs_of_words(v.to_words(nblocks * 2048))
