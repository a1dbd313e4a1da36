"""The operands of str_ref.json (string search over the planes of a bm::str_sparse_vector<>: find_eq_str and its batch forms,
src/bmsparsevec_algo.h:1194-1235, 2546-2588, 3263-3436) and the model the tests hold the device against.  Shared by
make_str_golden.py and the tests; every operand comes from fixed seeds and is held as the ascending positions of its ones.

A case is {"vecs": key -> (positions, nbits), "planes": [key or None, ...], "size": rows, "nn": key of the not-NULL vector or None,
"keys": (n, key_bytes) uint8 -- bit b of octet j of a key is plane 8 j + b (src/bmstrsparsevec.h:1423), zero padded --,
"entry_only": the queries that are no C string (a zero octet before a non-zero one): they go through the batch entry only}.

  model   row i < size spells octets[i, j] = sum over b of plane(8 j + b)[i] << b (absent plane, or past a plane's end: 0);
          key q matches row i iff the octets are equal byte for byte, both sides zero padded to the longer one; the all-zero key
          matches the all-zero rows that are not NULL (find_zero with null correction, :3412-3415)
          -> counts, found, first (the lowest row), and the ascending row list of every key

The reference shim exports no string container, so make_str_golden.py anchors every case in the reference through what it does
export (anchor_case): reference vectors built from the same planes, the AND-SUB group of every anchored key run through
ref_agg_pipeline_counts and ref_find_first_and_sub."""
from __future__ import annotations

import functools

import numpy as np

from import_cases import sha  # noqa: F401
from kleene_cases import K_BIT, K_FULL, K_GAP, K_NULL, _mixed, _vec  # noqa: F401
from rankc_cases import ones_of, oracle_vec, words_of  # noqa: F401

B = 65536
U = np.uint64
ALPHABET = b"acdeghiklmnoprstuvwy"                    # 20 letters
ANCHOR_KEYS = 200                                     # keys per case run through the reference (the first distinct ones)
GROUP_KEYS = 2                                        # keys per case whose AND / SUB plane lists the fixture records


def _case(vecs, planes, size, keys, nn=None, entry_only=()):
    keys = np.ascontiguousarray(keys, np.uint8)
    assert keys.ndim == 2
    return {"vecs": vecs, "planes": list(planes), "size": int(size), "nn": nn, "keys": keys, "entry_only": frozenset(entry_only)}


def pad(strs, width: int) -> np.ndarray:
    out = np.zeros((len(strs), width), np.uint8)
    for q, s in enumerate(strs):
        out[q, :len(s)] = np.frombuffer(bytes(s), np.uint8)
    return out


def _planes_of(octets: np.ndarray, nplanes: int, prefix: str = "p") -> dict:
    """octets: (rows, W) uint8 -> the plane vectors (all of `rows` bits)"""
    rows = octets.shape[0]
    return {"%s%d" % (prefix, p): (np.flatnonzero((octets[:, p >> 3] >> (p & 7)) & 1).astype(U), rows) for p in range(nplanes)}


def _words(rng, pool_size: int, lo: int, hi: int) -> list:
    """pool_size distinct strings of lo..hi letters"""
    out, seen = [], set()
    while len(out) < pool_size:
        n = int(rng.integers(lo, hi + 1))
        s = bytes(ALPHABET[i] for i in rng.integers(0, len(ALPHABET), n))
        if s not in seen:
            seen.add(s); out.append(s)
    return out


# ---- the cases ------------------------------------------------------------------------------------------------------------------------
def _grid():
    """14 block columns + 1,000 rows, 5 octets; per column the planes cycle through NULL / FULL / GAP / bit blocks; plane 13 is absent,
    plane 22 two blocks shorter than the column; a not-NULL vector.  Keys: what sampled rows spell, a duplicate, the empty string"""
    gs, nb, P = 14 * B + 1000, 15, 40
    vecs, planes = {}, []
    for p in range(P):
        if p == 13:
            planes.append(None); continue
        kinds = [(p + c) & 3 for c in range(nb)]
        vecs["p%d" % p] = _vec(kinds[:13], 900 + p, 13 * B) if p == 22 else _vec(kinds, 900 + p, gs)
        planes.append("p%d" % p)
    vecs["nn"] = _vec([(K_FULL, K_BIT, K_GAP)[c % 3] for c in range(nb)], 990, gs)
    case = _case(vecs, planes, gs, np.zeros((1, 5), np.uint8), "nn")
    octets = row_octets(case, 5)
    rows = [0, 1, 31, 32, 2047, 2048, 65535, 65536, 65537, 5 * B + 123, 12 * B + 7, 13 * B - 1, 13 * B, 13 * B + 40000, 14 * B, gs - 1]
    rows += list(np.random.default_rng(991).integers(0, gs, 40))
    keys = np.concatenate([octets[rows], octets[[5 * B + 123, 0]], np.zeros((1, 5), np.uint8)])
    ks = [bytes(k).rstrip(b"\0") for k in keys]
    return dict(case, keys=keys, entry_only=frozenset(q for q, k in enumerate(ks) if 0 in k))


def _sweep(P: int):
    """size = 2 * 65536 + 77 rows of P planes; the keys differ only in plane 31 or 32 (the tile boundary), only in the first
    octet, or only in the last"""
    size = 2 * B + 77
    W = (P + 7) // 8
    rng = np.random.default_rng(1000 + P)
    if P == 0:
        return _case({}, [], size, np.array([[1], [0], [0x80]], np.uint8))
    mask = np.full(W, 0xFF, np.uint8)
    if P & 7:
        mask[W - 1] = (1 << (P & 7)) - 1
    X = np.full(W, 0xA5, np.uint8) & mask
    if X[W - 1] == 0:
        X[W - 1] = 1
    variants = [X.copy()]

    def flip(plane):
        v = X.copy(); v[plane >> 3] ^= 1 << (plane & 7); return v
    if P > 31: variants.append(flip(31))
    if P > 32: variants.append(flip(32))
    if P > 1: variants.append(flip(1))                          # only the first octet
    variants.append(flip((W - 1) * 8))                           # only the last octet (its lowest bit)
    if P > 2: variants.append(flip(P - 1))                       # ... (the highest plane)
    absent = flip(0) if P > 8 else None                          # spelled by no row
    pick = rng.integers(0, len(variants) + 2, size)
    octets = np.zeros((size, W), np.uint8)
    for i, v in enumerate(variants):
        octets[pick == i] = v
    noise = pick >= len(variants)                                # X with two random planes flipped
    nz = np.flatnonzero(noise)
    octets[nz] = X
    for _ in range(2):
        pl = rng.integers(0, P, nz.size)
        octets[nz, pl >> 3] ^= (1 << (pl & 7)).astype(np.uint8)
    if absent is not None:
        octets[nz[np.all(octets[nz] == absent, axis=1)]] = X
    keys = np.array(variants + ([absent] if absent is not None else []) + [np.zeros(W, np.uint8)], np.uint8)
    ks = [bytes(k).rstrip(b"\0") for k in keys]
    return _case(_planes_of(octets, P), ["p%d" % p for p in range(P)], size, keys, None, [q for q, k in enumerate(ks) if 0 in k])


def _tail(size: int):
    """planes two blocks longer than the column spell the queried string in rows at and past `size`, inside the block that holds
    `size` and in the next one: none of those rows may count"""
    nrows = (size // B + 2) * B
    octets = pad([b"no"], 3).repeat(nrows, axis=0)
    K = np.frombuffer(b"yes", np.uint8)
    inside = [r for r in (0, size // 2, size - 1) if 0 <= r < size]
    beyond = [size, size + 1, size + 31, (size // B + 1) * B - 1, (size // B + 1) * B, nrows - 1]
    octets[sorted(set(inside + beyond))] = K
    return _case(_planes_of(octets, 24), ["p%d" % p for p in range(24)], size, pad([b"yes", b"no", b"ye", b""], 3))


@functools.lru_cache(maxsize=None)
def _pool_column():
    """2 * 65536 + 500 rows drawn from 3,000 strings of 1..6 letters in a 7-octet column; some rows are empty, some of those NULL;
    rows 10 / 11 hold "ab" / "abc"; plane 55 is absent (no row needs it)"""
    rng = np.random.default_rng(1100)
    size = 2 * B + 500
    pool = _words(rng, 3000, 1, 6)
    for s in (b"ab", b"abc"):
        if s in pool: pool.remove(s)
    pool = pool[:2998] + [b"ab", b"abc"]
    pick = rng.integers(0, 2998, size)                      # ("ab" and "abc" are in rows 10 and 11 only)
    pick[10], pick[11] = 2998, 2999
    octets = pad(pool, 7)[pick]
    empty = rng.random(size) < 0.01
    empty[[10, 11]] = False
    octets[empty] = 0
    null = empty & (rng.random(size) < 0.5)
    vecs = _planes_of(octets, 55)
    vecs["nn"] = (np.flatnonzero(~null).astype(U), size)
    return vecs, ["p%d" % p for p in range(55)] + [None], size, pool


def _pool_case(keys, nn=True, entry_only=()):
    vecs, planes, size, _ = _pool_column()
    return _case(vecs, planes, size, keys, "nn" if nn else None, entry_only)


@functools.lru_cache(maxsize=None)
def _dictionary():
    """70,000 distinct strings of 6..16 letters, one per row, queried with all of them, shuffled"""
    rng = np.random.default_rng(1200)
    words = _words(rng, 70000, 6, 16)
    octets = pad(words, 16)
    return _case(_planes_of(octets, 128), ["p%d" % p for p in range(128)], len(words), octets[rng.permutation(len(words))])


def _first():
    """"first" sits in columns 0, 5 and 13, twice inside one 32-row word of column 0; "later" only in column 13, twice in one word"""
    rng = np.random.default_rng(1300)
    size = 14 * B
    pool = pad(_words(rng, 500, 2, 8), 8)
    octets = pool[rng.integers(0, 500, size)]
    octets[[7000, 7003, 5 * B + 1, 13 * B + 500]] = pad([b"first"], 8)
    octets[[13 * B + 9, 13 * B + 12]] = pad([b"later"], 8)
    return _case(_planes_of(octets, 64), ["p%d" % p for p in range(64)], size, pad([b"later", b"first", b"never", b"firs"], 8))


@functools.lru_cache(maxsize=None)
def cases():
    c = {"grid": _grid()}
    for P in (0, 1, 8, 31, 32, 33, 64, 65, 72, 256, 257):
        c["planes_%d" % P] = _sweep(P)
    for size in (1, 31, 32, 33, 63, 64, 65, 2047, 2048, 2049, 65535, 65536, 65537):
        c["tail_%d" % size] = _tail(size)
    pool = _pool_column()[3]
    rng = np.random.default_rng(1101)
    for n in (0, 1, 2, 64, 65, 300, 3000):
        c["keys_n%d" % n] = _pool_case(pad([pool[i] for i in rng.permutation(len(pool))[:n]], 7))
    c["keys_duplicates"] = _pool_case(pad([pool[5], pool[6], pool[5], b"", pool[5], b"", pool[6]], 7))
    c["keys_empty_with_nn"] = _pool_case(pad([b"", pool[1]], 7))
    c["keys_empty_without_nn"] = _pool_case(pad([b"", pool[1]], 7), nn=False)
    c["keys_absent_plane"] = _pool_case(pad([pool[2][:1] + b"\0" * 5 + b"\x80", pool[2]], 7), entry_only=[0])     # bit 7 of octet 6 = plane 55
    c["keys_wider_zero_tail"] = _pool_case(pad([pool[3], b"ab"], 12))
    c["keys_wider_nonzero_tail"] = _pool_case(pad([pool[3] + b"\0" * (11 - len(pool[3])) + b"a", b"ab" + b"\0" * 9 + b"\x01", b"ab"], 12), entry_only=[0, 1])
    c["keys_narrower"] = _pool_case(pad([b"ab", b"a", b"abc"], 3))
    c["dictionary"] = _dictionary()
    one = pad([b"hello"], 5).repeat(2 * B + 77, axis=0)
    c["every_row"] = _case(_planes_of(one, 40), ["p%d" % p for p in range(40)], 2 * B + 77, pad([b"hello", b"hellp", b"hell"], 5))
    c["first"] = _first()
    return c


# ---- the model ------------------------------------------------------------------------------------------------------------------------
def _bits(case: dict, key, n: int) -> np.ndarray:
    out = np.zeros(n, bool)
    if key is not None:
        ids = case["vecs"][key][0]
        out[ids[ids < U(n)].astype(np.int64)] = True
    return out


def row_octets(case: dict, width: int) -> np.ndarray:
    """(size, width) uint8: what the planes spell in every row of the column"""
    n, P = case["size"], len(case["planes"])
    width = max(width, (P + 7) // 8, 1)
    out = np.zeros((n, width), np.uint8)
    for p, k in enumerate(case["planes"]):
        if k is not None:
            out[:, p >> 3] |= _bits(case, k, n).astype(np.uint8) << (p & 7)
    return out


def model_case(case: dict) -> dict:
    """-> counts, found, first (uint64 / bool / uint64 per key) and offsets, ids: the ascending rows of every key, back to back"""
    keys = case["keys"]
    nq = keys.shape[0]
    octets = row_octets(case, keys.shape[1])
    W = octets.shape[1]
    n = case["size"]
    valid = np.ones(n, bool)
    if case["nn"] is not None:
        valid = _bits(case, case["nn"], n) | octets.any(axis=1)          # (the not-NULL vector bears on the all-zero rows only)
    rows = np.flatnonzero(valid)
    uniq, inverse = (np.unique(octets[rows], axis=0, return_inverse=True) if rows.size else (np.zeros((0, W), np.uint8), np.zeros(0, np.int64)))
    inverse = np.asarray(inverse).reshape(-1)
    order = np.argsort(inverse, kind="stable")
    starts = np.searchsorted(inverse[order], np.arange(uniq.shape[0] + 1))
    index = {uniq[i].tobytes(): i for i in range(uniq.shape[0])}
    parts = []
    for q in range(nq):
        k = np.zeros(W, np.uint8); k[:keys.shape[1]] = keys[q]
        i = index.get(k.tobytes())
        parts.append(rows[order[starts[i]:starts[i + 1]]].astype(U) if i is not None else np.zeros(0, U))
    counts = np.array([p.size for p in parts], U)
    offsets = np.zeros(nq + 1, U)
    offsets[1:] = np.cumsum(counts, dtype=U)
    return {"counts": counts, "found": counts > 0, "first": np.array([p[0] if p.size else 0 for p in parts], U),
            "offsets": offsets, "ids": np.concatenate(parts) if parts else np.zeros(0, U)}


def loop_case(case: dict) -> dict:
    """the same by a plain loop over keys and rows (small cases only)"""
    keys = case["keys"]
    octets = row_octets(case, keys.shape[1])
    W = octets.shape[1]
    nn = _bits(case, case["nn"], case["size"]) if case["nn"] is not None else None
    counts, first = [], []
    for q in range(keys.shape[0]):
        k = bytes(keys[q]) + b"\0" * (W - keys.shape[1])
        hits = []
        for i in range(case["size"]):
            if bytes(octets[i]) == k and (any(k) or nn is None or nn[i]):
                hits.append(i)
        counts.append(len(hits)); first.append(hits[0] if hits else 0)
    return {"counts": np.array(counts, U), "first": np.array(first, U)}


def key_strings(case: dict) -> list:
    """the keys as the strings a caller passes (trailing padding removed)"""
    return [bytes(k).rstrip(b"\0") for k in case["keys"]]


def groups_of(case: dict, builder, prefix_sub: bool = True) -> list:
    """[query, [AND planes, SUB planes] or None] of the first GROUP_KEYS C-string keys, by `builder`
    (bitmagic_amd.str_search_groups); a plane list is its numbers in order, joined by blanks"""
    present = [k is not None for k in case["planes"]]
    out = []
    for q, s in enumerate(key_strings(case)):
        if q in case["entry_only"] or not s:
            continue
        g = builder(s, present, prefix_sub)
        out.append([q, None if g is None else [" ".join(map(str, g[0])), " ".join(map(str, g[1]))]])
        if len(out) == GROUP_KEYS:
            break
    return out


def record(case: dict, m: dict, builder) -> dict:
    return {"n": int(m["counts"].size), "hits": int(m["counts"].sum()), "n_found": int(m["found"].sum()),
            "counts_sha": sha(m["counts"].astype("<u8")), "first_sha": sha(m["first"].astype("<u8")),
            "offsets_sha": sha(m["offsets"].astype("<u8")), "ids_sha": sha(m["ids"].astype("<u8")),
            "groups": groups_of(case, builder, True), "groups_prefix": groups_of(case, builder, False)}


# ---- the model against the reference (generator only) -------------------------------------------------------------------------------
def anchor_case(R, case: dict, m: dict, builder) -> dict:
    """reference vectors from the same planes; the AND-SUB group of each of the first ANCHOR_KEYS distinct keys through the
    reference's counts pipeline and find_first_and_sub (the empty string: AND = [0, size) and the not-NULL vector, SUB = every
    plane); the model must give the same counts and first rows"""
    n = case["size"]
    rv = {k: oracle_vec(R, ids, max(nbits, 1)) for k, (ids, nbits) in case["vecs"].items()}
    present = [k is not None for k in case["planes"]]
    rows = oracle_vec(R, np.arange(n, dtype=U), max(n, 1)) if n else None
    groups, which, seen = [], [], set()
    for q, s in enumerate(key_strings(case)):
        if s in seen or len(groups) == ANCHOR_KEYS:
            continue
        seen.add(s)
        if s:
            g = builder(s, present, True)
            if g is None:
                assert m["counts"][q] == 0, ("a key without its planes matched", q)
                continue
            if rows is None:
                assert m["counts"][q] == 0
                continue
            # (a container's planes end with its rows; a case's planes may be longer: the column's rows join the AND list)
            a, sub = [rv[case["planes"][p]] for p in g[0]] + [rows], [rv[case["planes"][p]] for p in g[1]]
        else:
            if rows is None:
                assert m["counts"][q] == 0
                continue
            a = [rows] + ([rv[case["nn"]]] if case["nn"] is not None else [])
            sub = [rv[k] for k in case["planes"] if k is not None]
        groups.append((a, sub)); which.append(q)
    if groups:
        cnt = R.pipeline_counts(groups)
        for (a, sub), q, c in zip(groups, which, cnt):
            assert int(c) == int(m["counts"][q]), ("count", q, int(c), int(m["counts"][q]))
            if len(a) == 1 and not sub:
                # the empty string over a column without planes and without a not-NULL vector: the group is the vector [0, size)
                # itself, its first row is read from it (for a lone vector that starts with a FULL block the reference's
                # find_first_and_sub answers 4, not 0: no other search builds such a group)
                f, idx = True, int(ones_of(a[0])[0])
            else:
                f, idx = R.find_first_and_sub(a, sub)
            assert bool(f) == bool(m["found"][q]) and (not f or idx == int(m["first"][q])), ("first", q, f, idx)
    return {"keys": len(groups), "hits": int(sum(int(m["counts"][q]) for q in which))}


# ---- the same operands on the device -------------------------------------------------------------------------------------------------
def device_scanner(bm, ctx, case: dict):
    """-> (str_scanner, vecs)"""
    vecs = {k: bm.bit_import_u32(ctx, words_of(ids, max(nbits, 1)), True) for k, (ids, nbits) in case["vecs"].items()}
    sc = bm.str_scanner(ctx, [vecs[k] if k is not None else None for k in case["planes"]], size=case["size"],
                        not_null=vecs[case["nn"]] if case["nn"] is not None else None)
    return sc, vecs
