"""The operands of kleene_ref.json (bm::and_kleene / bm::or_kleene, src/bm3vl.h:151-262) and the two ways the tests restate the
reference.  Shared by make_kleene_golden.py and the tests; every operand comes from fixed seeds and is held as the ascending
positions of its ones.  The canonical form of a block table is import_cases.record().

A case is {"vecs": key -> (positions, nbits), "pairs": [(value key, not-NULL key), ...]}: the same key is the same vector (one
handle on the device).  Both operations are applied to every case; a list is folded from the left with the in-place form.

  oracle_*   the reference's own eight-step sequence (:186-197 OR, :250-261 AND) through Oracle.op2 -- every call those
             functions make -- of the reference or of the C port, then optimize() and flatten
  model_*    the per-bit rules on unpacked bits:
               AND:  V = v1 & v2    amb = n1 ^ n2    N = (n1 | n2) & ~(amb & v1) & ~(amb & v2)
               OR:   V = v1 | v2                     N = (n1 | n2) & ~((v1 ^ n1) & ~n2) & ~((v2 ^ n2) & ~n1)"""
from __future__ import annotations

import functools

import numpy as np

from import_cases import _alternating, record, sha  # noqa: F401
from rankc_cases import _cat, _full, _rand, _runs, ones_of, words_of  # noqa: F401

B = 65536
U = np.uint64
AND, OR, XOR, SUB = 0, 1, 2, 3
OPS = {"and": AND, "or": OR}
K_NULL, K_FULL, K_GAP, K_BIT = 0, 1, 2, 3            # the kind codes of a case's block plan (not the table's)


def _block(kind: int, seed: int, b: int) -> np.ndarray:
    if kind == K_NULL:
        return np.zeros(0, U)
    if kind == K_FULL:
        return _full(b)
    if kind == K_GAP:                                   # sparse bits or long runs: a GAP block either way
        return _rand(seed, b, 0.002) if seed & 1 else _runs(b, seed, 40)
    return _rand(seed, b, 0.3)


def _vec(kinds, seed: int, nbits: int | None = None):
    ids = _cat(*[_block(int(k), seed * 1000 + b, b) for b, k in enumerate(kinds)])
    nbits = len(kinds) * B if nbits is None else nbits
    return ids[ids < U(nbits)], int(nbits)


def _mixed(seed: int, nblocks: int, nbits: int | None = None):
    return _vec(np.random.default_rng(seed).integers(0, 4, nblocks), seed, nbits)


def _inside(v, n):
    """init_kleene (:53): v &= n"""
    return np.intersect1d(v[0], n[0], assume_unique=True), v[1]


def _quadruple():
    nb = 256
    nbits = nb * B - 77
    ks = [[(b >> s) & 3 for b in range(nb)] for s in (0, 2, 4, 6)]
    return {k: _vec(ks[i], 11 + i, nbits) for i, k in enumerate(("v1", "n1", "v2", "n2"))}


@functools.lru_cache(maxsize=None)
def cases():
    c = {}
    q = _quadruple()
    two = [("v1", "n1"), ("v2", "n2")]
    c["every_kind_quadruple"] = {"vecs": q, "pairs": two}
    c["initialised"] = {"vecs": dict(q, v1=_inside(q["v1"], q["n1"]), v2=_inside(q["v2"], q["n2"])), "pairs": two}
    # results of exactly 1,275 and 1,276 runs (the GAP limit of optimize()), in both outputs of both operations
    a5 = lambda b: _alternating(b, 1, 637)
    a6 = lambda b: _alternating(b, 0, 638)
    c["gap_threshold"] = {"vecs": {
        "v1": (_cat(a5(0), a6(1), a5(2), a6(3), a5(6), a6(7)), 8 * B),
        "n1": (_cat(_full(0), _full(1), _full(2), _full(3), a5(4), a6(5), a5(6), a6(7)), 8 * B),
        "v2": (_cat(_full(0), _full(1)), 8 * B),
        "n2": (_cat(_full(0), _full(1), _full(2), _full(3)), 8 * B)}, "pairs": two}
    r = lambda seed: _cat(*[_rand(seed + b, b, 0.3) for b in range(3)])
    c["all_unknown"] = {"vecs": {"v1": (r(20), 3 * B), "v2": (r(30), 3 * B), "n": (np.zeros(0, U), 3 * B)}, "pairs": [("v1", "n"), ("v2", "n")]}
    c["all_known"] = {"vecs": {"v1": (r(40), 3 * B), "v2": (r(50), 3 * B), "n": (_cat(_full(0), _full(1), _full(2)), 3 * B)},
                      "pairs": [("v1", "n"), ("v2", "n")]}
    c["value_is_null_vector"] = {"vecs": {"a": _mixed(60, 5), "v2": _mixed(61, 5), "n2": _mixed(62, 5)}, "pairs": [("a", "a"), ("v2", "n2")]}
    c["ragged_1_3_8"] = {"vecs": {"v1": _mixed(70, 1), "n1": _mixed(71, 3), "v2": _mixed(72, 8), "n2": _mixed(73, 3, 3 * B - 1000)}, "pairs": two}
    five = lambda bits: (np.array(bits, U), 5)
    c["five_bits"] = {"vecs": {"v1": five([0, 1, 4]), "n1": five([0, 1, 2]), "v2": five([1, 3, 4]), "n2": five([1, 2, 4])}, "pairs": two}
    # fold lists: pairs drawn from a pool of mixed-kind vectors of 1, 3, 5 and 8 blocks; fold_3 repeats its first pair
    pool = {"p%d" % i: _mixed(80 + i, (1, 3, 5, 8)[i & 3], None if i % 5 else (1, 3, 5, 8)[i & 3] * B - 4321) for i in range(12)}
    pool["e"] = (np.zeros(0, U), 2 * B)
    keys = sorted(pool)
    for n in (1, 2, 5, 17):
        pick = np.random.default_rng(90 + n).integers(0, len(keys), (n, 2))
        pairs = [(keys[i], keys[j]) for i, j in pick]
        used = {k for p in pairs for k in p}
        c["fold_%d" % n] = {"vecs": {k: pool[k] for k in used}, "pairs": pairs}
    c["fold_3_repeats_a_pair"] = {"vecs": {k: pool[k] for k in ("p2", "p7", "p3", "p6")}, "pairs": [("p2", "p7"), ("p3", "p6"), ("p2", "p7")]}
    return c


def case_nbits(case: dict) -> int:
    return max(nbits for _, nbits in case["vecs"].values())


# ---- the reference's sequences through an oracle (the reference or the C port): op2 and nothing else -------------------------
def oracle_and(o, v1, n1, v2, n2):
    """and_kleene (:250-261)"""
    amb1 = o.op2(XOR, n1, n2)
    amb2 = amb1                                                   # ("just a copy")
    amb1 = o.op2(AND, amb1, v1)
    amb2 = o.op2(AND, amb2, v2)
    vt = o.op2(AND, v1, v2)
    nt = o.op2(OR, n1, n2)
    nt = o.op2(SUB, nt, amb1)
    nt = o.op2(SUB, nt, amb2)
    return vt, nt


def oracle_or(o, v1, n1, v2, n2):
    """or_kleene (:186-197)"""
    kf1 = o.op2(XOR, v1, n1)
    kf2 = o.op2(XOR, v2, n2)
    kf1 = o.op2(SUB, kf1, n2)
    kf2 = o.op2(SUB, kf2, n1)
    vt = o.op2(OR, v1, v2)
    nt = o.op2(OR, n1, n2)
    nt = o.op2(SUB, nt, kf1)
    nt = o.op2(SUB, nt, kf2)
    return vt, nt


def oracle_fold(o, op: int, pairs):
    """pairs: [(value Vec, not-NULL Vec)] -> the left fold, as the in-place overloads (:151, :213) give it"""
    step = oracle_and if op == AND else oracle_or
    v, n = pairs[0]
    for v2, n2 in pairs[1:]:
        v, n = step(o, v, n, v2, n2)
    return v, n


def _oracle_out(vec, nbits: int) -> dict:
    vec.nbits = nbits
    vec.optimize()                                                # (a list of one pair: its operands are optimised already)
    return {"nbits": int(nbits), "count": int(vec.count()), "opt1": record(*vec.flatten()), "ids_sha": sha(ones_of(vec).astype("<u8"))}


def oracle_case(o, case: dict) -> dict:
    from rankc_cases import oracle_vec
    nbits = case_nbits(case)
    vecs = {k: oracle_vec(o, ids, nb) for k, (ids, nb) in case["vecs"].items()}
    out = {"npairs": len(case["pairs"]), "nbits": nbits}
    for name, op in OPS.items():
        v, n = oracle_fold(o, op, [(vecs[a], vecs[b]) for a, b in case["pairs"]])
        rv, rn = _oracle_out(v, nbits), _oracle_out(n, nbits)
        t, f = int(o.count_op2(AND, n, v)), int(o.count_op2(SUB, n, v))
        out[name] = {"value": rv, "null": rn, "counts": [f, nbits - int(n.count()), t]}
    return out


# ---- the per-bit rules on unpacked bits ------------------------------------------------------------------------------------------
def bits_of(ids: np.ndarray, nblocks: int) -> np.ndarray:
    bits = np.zeros(nblocks * B, bool)
    bits[ids.astype(np.int64)] = True
    return bits


def model_step(op: int, V, N, x, y):
    if op == AND:
        amb = N ^ y
        return V & x, (N | y) & ~(amb & V) & ~(amb & x)
    return V | x, (N | y) & ~((V ^ N) & ~y) & ~((x ^ y) & ~N)


def model_fold(op: int, case: dict):
    """-> (V bits, N bits) over whole blocks of the largest operand"""
    nblocks = (case_nbits(case) + B - 1) // B
    bits = {k: bits_of(ids, nblocks) for k, (ids, _) in case["vecs"].items()}
    (a, b), rest = case["pairs"][0], case["pairs"][1:]
    V, N = bits[a], bits[b]
    for a, b in rest:
        V, N = model_step(op, V, N, bits[a], bits[b])
    return V, N


def table_of_bits(bits: np.ndarray, optimize: bool) -> dict:
    """record() of the table the storage rule gives: no bit -> NULL, all 65,536 -> FULL; optimize: fewer than 1,276 runs a
    GAP block (blocks_manager::optimize_bit_block, src/bmblocks.h:1412-1436), else a bit-block; without: a bit-block"""
    blocks = bits.reshape(-1, B)
    nblocks = blocks.shape[0]
    kinds = np.zeros(nblocks, np.uint8); offs = np.zeros(nblocks, np.uint32)
    pop = blocks.sum(axis=1)
    bit_parts, gap_parts, gpos = [], [], 0
    for b in range(nblocks):
        if pop[b] == 0:
            continue
        if pop[b] == B:
            kinds[b] = 1
            continue
        ends = np.flatnonzero(blocks[b, 1:] != blocks[b, :-1]).astype(np.uint16)
        runs = ends.size + 1
        if optimize and runs < 1276:
            kinds[b] = 3; offs[b] = gpos
            g = np.concatenate([[np.uint16((runs << 3) | int(blocks[b, 0]))], ends, [np.uint16(65535)]]).astype(np.uint16)
            gap_parts.append(g); gpos += g.size
        else:
            kinds[b] = 2; offs[b] = len(bit_parts)
            bit_parts.append(np.packbits(blocks[b], bitorder="little").view(np.uint32))
    return record(kinds, offs, np.concatenate(bit_parts) if bit_parts else np.zeros(0, np.uint32),
                  np.concatenate(gap_parts) if gap_parts else np.zeros(0, np.uint16))


@functools.lru_cache(maxsize=None)
def model_case(name: str) -> dict:
    """what the fixture holds per operation, from the rules alone, and the table without optimize ("opt0")"""
    case = cases()[name]
    nbits = case_nbits(case)
    out = {"npairs": len(case["pairs"]), "nbits": nbits}
    for opname, op in OPS.items():
        V, N = model_fold(op, case)
        r = {}
        for key, bits in (("value", V), ("null", N)):
            pos = np.flatnonzero(bits).astype("<u8")
            r[key] = {"nbits": nbits, "count": int(pos.size), "opt1": table_of_bits(bits, True), "opt0": table_of_bits(bits, False),
                      "ids_sha": sha(pos)}
        r["counts"] = [int((N & ~V).sum()), nbits - int(N.sum()), int((N & V).sum())]
        out[opname] = r
    return out
