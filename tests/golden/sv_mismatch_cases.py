"""The operands of sv_mismatch_ref.json (bm::sparse_vector_find_mismatch, src/bmsparsevec_algo.h:656-792, and
bm::sparse_vector_find_first_mismatch, :478-636) and the two ways the tests restate the reference.  Shared by
make_sv_mismatch_golden.py and the tests; every operand comes from fixed seeds and is held as the ascending positions of its ones.

A case is {"vecs": key -> (positions, nbits), "a": column, "b": column, "bit_keys": keys stored as bit-blocks whatever they hold}
with column = {"planes": [key or None, ...], "size": rows, "nn": key of the not-NULL vector or None}: the same key is the same
vector (one handle on the device).  Every case is evaluated under both null_proc values.

  replay_*   the reference's own sequence of whole-vector calls from the lines above through Oracle.op2, Vec.set_range and
             Oracle.find_first of the reference or of the C port.  invert() of a resized vector is ones[0, size) SUB N; the first
             mismatch is find_first of the XORs, minimised as the reference does.
  model_*    no planes: value_a[i] != value_b[i] on the rows' values, then the size and NULL rules on unpacked bits.

use_null without a not-NULL vector on either side has no vector result (the reference sets every position up to id_max there;
the device entry returns BMX_ERR_BADARG): the fixture holds null for its count and hash."""
from __future__ import annotations

import functools

import numpy as np

from import_cases import sha  # noqa: F401
from kleene_cases import K_BIT, K_FULL, K_GAP, K_NULL, _mixed, _vec  # noqa: F401
from rankc_cases import _cat, _rand, ones_of, oracle_vec, words_of  # noqa: F401

B = 65536
U = np.uint64
AND, OR, XOR, SUB = 0, 1, 2, 3
USE_NULL, NO_NULL = 0, 1
PROCS = {"use_null": USE_NULL, "no_null": NO_NULL}
ID_MAX = 0xFFFFFFFF


def _col(planes, size, nn=None):
    return {"planes": list(planes), "size": int(size), "nn": nn}


def _case(vecs, a, b, bit_keys=(), values=None):
    return {"vecs": vecs, "a": a, "b": b, "bit_keys": frozenset(bit_keys), "values": values}


def _cut(v, nbits):
    ids, _ = v
    return ids[ids < U(nbits)], int(nbits)


def _ones(n):
    return np.arange(n, dtype=U), int(n)


def _flip(v, positions):
    """the vector with the given positions inverted"""
    ids, nbits = v
    return np.setxor1d(ids, np.asarray(positions, U)).astype(U), nbits


def _grid():
    """every pair of block kinds for (A_0, B_0) over 16 columns; plane 1 carries the transposed plan"""
    size = 16 * B - 77
    ka = [c & 3 for c in range(16)]
    kb = [c >> 2 for c in range(16)]
    return {"a0": _vec(ka, 201, size), "b0": _vec(kb, 202, size), "a1": _vec(kb, 203, size), "b1": _vec(ka, 204, size)}, size


def _value_columns():
    rows = 3 * B - 1000
    rng = np.random.default_rng(310)
    va = rng.integers(0, 1 << 32, rows, dtype=np.uint64).astype(np.uint32)
    null_a = rng.random(rows) < 0.05
    vb = va.copy()
    ch = rng.choice(rows, size=300, replace=False)
    vb[ch] = rng.integers(0, 1 << 32, 300, dtype=np.uint64).astype(np.uint32)
    null_b = null_a.copy()
    fl = rng.choice(rows, size=50, replace=False)
    null_b[fl] = ~null_b[fl]
    va[null_a] = 0; vb[null_b] = 0                                   # NULL elements are stored as 0
    vecs = {}
    for side, v, nl in (("a", va, null_a), ("b", vb, null_b)):
        for i in range(32):
            vecs["%s%d" % (side, i)] = (np.flatnonzero((v >> np.uint32(i)) & np.uint32(1)).astype(U), rows)
        vecs["n" + side] = (np.flatnonzero(~nl).astype(U), rows)
    return vecs, rows, (va, vb, null_a, null_b)


@functools.lru_cache(maxsize=None)
def cases():
    c = {}
    # ---- block-kind grid, without and with two not-NULL vectors of mixed kinds
    g, gs = _grid()
    c["grid"] = _case(g, _col(["a0", "a1"], gs), _col(["b0", "b1"], gs))
    gn = dict(g, na=_cut(_mixed(205, 16), gs), nb=_cut(_mixed(206, 16), gs))
    c["grid_nn"] = _case(gn, _col(["a0", "a1"], gs, "na"), _col(["b0", "b1"], gs, "nb"))
    # ---- real value columns: 32 planes by bit slicing, b = a except in a few hundred rows
    vv, rows, values = _value_columns()
    c["values_32"] = _case(vv, _col(["a%d" % i for i in range(32)], rows, "na"), _col(["b%d" % i for i in range(32)], rows, "nb"), values=values)
    # ---- ragged plane counts: 5 against 9, absent planes on either side
    rs = 3 * B - 4321
    rv = {"a%d" % i: _cut(_mixed(220 + i, 3), rs) for i in (0, 1, 3, 4)}
    rv.update({"b%d" % i: _cut(_mixed(230 + i, 3), rs) for i in (1, 2, 3, 4, 5, 6, 8)})
    rv["b3"] = rv["a3"]                                               # (one equal pair of distinct handles)
    rv.update(na=_cut(_mixed(240, 3), rs), nb=_cut(_mixed(241, 3), rs))
    c["ragged_5_9"] = _case(rv, _col(["a0", "a1", None, "a3", "a4"], rs, "na"),
                            _col([None, "b1", "b2", "b3", "b4", "b5", "b6", None, "b8"], rs, "nb"))
    c["ragged_9_5"] = _case(rv, c["ragged_5_9"]["b"], c["ragged_5_9"]["a"])
    # ---- 64 planes of one column each
    ps = B - 100
    pv = {"a%d" % i: _cut(_mixed(300 + i, 1), ps) for i in range(64)}
    for i in range(64):                                               # b: the same planes with a few rows changed in every fourth
        pv["b%d" % i] = _flip(pv["a%d" % i], [7 * i, 1000 + i]) if i % 4 == 0 else pv["a%d" % i]
    pv.update(na=_cut(_mixed(390, 1), ps), nb=_cut(_mixed(391, 1), ps))
    c["planes_64"] = _case(pv, _col(["a%d" % i for i in range(64)], ps, "na"), _col(["b%d" % i for i in range(64)], ps, "nb"))
    # ---- size difference inside one block and across blocks, with both, one (each side) and no not-NULL vector
    for name, sa, sb in (("size_in_block", B + 100, B + 5000), ("size_across", B - 3, 4 * B + 17)):
        nba, nbb = (sa + B - 1) // B, (sb + B - 1) // B
        sv = {"a0": _cut(_mixed(400, nba), sa), "a1": _cut(_mixed(401, nba), sa), "a2": _cut(_mixed(402, nba), sa)}
        sv["b0"] = _cut(_mixed(400, nbb), sb)                        # (the same seed: equal below a's size)
        sv["b1"] = _cut(_mixed(411, nbb), sb); sv["b2"] = _cut(_mixed(402, nbb), sb)
        sv.update(na=_cut(_mixed(420, nba), sa), nb=_cut(_mixed(423, nbb), sb))
        for tag, na_, nb_ in (("both", "na", "nb"), ("only_a", "na", None), ("only_b", None, "nb"), ("none", None, None)):
            c["%s_%s" % (name, tag)] = _case(sv, _col(["a0", "a1", "a2"], sa, na_), _col(["b0", "b1", "b2"], sb, nb_))
            c["%s_swapped_%s" % (name, tag)] = _case(sv, _col(["b0", "b1", "b2"], sb, nb_), _col(["a0", "a1", "a2"], sa, na_))
    # ---- equal content
    es = 5 * B - 10
    ev = {"p0": _cut(_mixed(500, 5), es), "p1": _cut(_mixed(501, 5), es), "n": _cut(_mixed(502, 5), es)}
    c["same_handles"] = _case(ev, _col(["p0", "p1"], es, "n"), _col(["p0", "p1"], es, "n"))
    gv = {"g0": _cut(_vec([K_GAP] * 3, 510), 3 * B - 5), "g1": _cut(_vec([K_GAP, K_NULL, K_GAP], 511), 3 * B - 5), "n": _ones(3 * B - 5)}
    gv["r0"], gv["r1"] = gv["g0"], gv["g1"]                          # the same ones, kept as bit-blocks
    c["equal_gap_vs_bit"] = _case(gv, _col(["g0", "g1"], 3 * B - 5, "n"), _col(["r0", "r1"], 3 * B - 5, "n"), bit_keys=("r0", "r1"))
    fs = 2 * B + 500
    fv = {"f0": _ones(fs), "f1": _ones(fs), "n": _ones(fs)}
    c["all_rows_differ"] = _case(fv, _col(["f0", "f1"], fs, "n"), _col([], fs, "n"))
    # ---- small and empty inputs
    five = lambda bits: (np.array(bits, U), 5)
    c["five_rows"] = _case({"a0": five([0, 1, 4]), "a1": five([2]), "b0": five([0, 4]), "b1": five([2, 3]), "na": five([0, 1, 2, 4]), "nb": five([0, 1, 2, 3])},
                           _col(["a0", "a1"], 5, "na"), _col(["b0", "b1"], 5, "nb"))
    c["size_zero"] = _case({"a0": five([]), "b0": five([]), "n": five([])}, _col(["a0"], 0, "n"), _col(["b0"], 0, "n"))
    c["no_planes"] = _case({"n": _ones(B + 9)}, _col([], B + 9, "n"), _col([], B + 9, "n"))
    # ---- first-mismatch placement
    ms = 2 * B + 99
    mv = {"p0": _cut(_mixed(600, 3), ms), "p1": _cut(_mixed(601, 3), ms), "n": _cut(_mixed(602, 3), ms)}
    mv["q_row0"] = _flip(mv["p1"], [0])
    mv["q_last"] = _flip(mv["p1"], [ms - 1])
    mv["n_diff"] = _flip(mv["n"], [B + 4242])
    c["first_at_row0"] = _case(mv, _col(["p0", "p1"], ms, "n"), _col(["p0", "q_row0"], ms, "n"))
    c["first_at_last_row"] = _case(mv, _col(["p0", "p1"], ms, "n"), _col(["p0", "q_last"], ms, "n"))
    c["first_only_in_not_null"] = _case(mv, _col(["p0", "p1"], ms, "n"), _col(["p0", "p1"], ms, "n_diff"))
    ls = 40 * B - 1
    lv = {"p0": _cut(_vec([K_GAP, K_BIT, K_NULL, K_FULL] * 10, 610), ls), "p1": _cut(_vec([K_GAP] * 40, 611), ls), "n": _ones(ls)}
    lv["q0"] = _flip(lv["p0"], [39 * B + 31337])
    c["first_in_last_of_40_columns"] = _case(lv, _col(["p0", "p1"], ls, "n"), _col(["q0", "p1"], ls, "n"))
    # only beyond the shorter column: equal planes, b has more rows (all of value 0)
    bs, bl = B + 700, 2 * B + 300
    bv = {"p0": _cut(_mixed(620, 2), bs), "p1": _cut(_mixed(621, 2), bs), "ns": _ones(bs), "nl": _ones(bl)}
    c["beyond_shorter_none"] = _case(bv, _col(["p0", "p1"], bs), _col(["p0", "p1"], bl))
    c["beyond_shorter_both"] = _case(bv, _col(["p0", "p1"], bs, "ns"), _col(["p0", "p1"], bl, "nl"))
    return c


def case_size(case: dict) -> int:
    return max(case["a"]["size"], case["b"]["size"])


def has_vector_result(case: dict, proc: int) -> bool:
    return not (proc == USE_NULL and case["a"]["nn"] is None and case["b"]["nn"] is None)


def case_words(case: dict, key: str) -> np.ndarray:
    ids, nbits = case["vecs"][key]
    return words_of(ids, max(nbits, 1))


# ---- the reference's sequences through an oracle (the reference or the C port) ---------------------------------------------------
def _oracle_vecs(o, case: dict) -> dict:
    out = {}
    for k, (ids, nbits) in case["vecs"].items():
        nbits = max(nbits, 1)
        out[k] = o.import_words(words_of(ids, nbits), False, nbits) if k in case["bit_keys"] else oracle_vec(o, ids, nbits)
    return out


def _ones_vec(o, n: int, nbits: int):
    v = o.new(max(nbits, 1))
    if n:
        v.set_range(0, n - 1)
    return v


def replay_mismatch(o, pa, sa, na, pb, sb, nb, proc: int):
    """sparse_vector_find_mismatch (:656-792) -> Vec, or None where no vector can hold the result"""
    hi = max(sa, sb)
    bv = o.new(max(hi, 1))
    for i in range(max(len(pa), len(pb))):                            # :686-714
        b1 = pa[i] if i < len(pa) else None
        b2 = pb[i] if i < len(pb) else None
        if b1 is None:
            if b2 is not None:
                bv = o.op2(OR, bv, b2)
            continue
        if b2 is None:
            bv = o.op2(OR, bv, b1)
            continue
        bv = o.op2(OR, bv, o.op2(XOR, b1, b2))
    if sa != sb:                                                      # :716-731
        bv.set_range(min(sa, sb), hi - 1)
    if proc == NO_NULL:                                               # :740-759
        if na is not None and nb is not None:
            bv = o.op2(AND, bv, o.op2(OR, na, nb))
        else:
            if na is not None:
                bv = o.op2(AND, bv, na)
            if nb is not None:
                bv = o.op2(AND, bv, nb)
    else:                                                             # :760-788
        if na is not None and nb is not None:
            bv = o.op2(OR, bv, o.op2(XOR, na, nb))
        elif na is None and nb is None:
            return None                                               # invert() of an empty vector: every position up to id_max
        else:
            n, size = (na, sa) if nb is None else (nb, sb)            # (:775-784: bv_null = *N; resize(size); invert())
            bv = o.op2(OR, bv, o.op2(SUB, _ones_vec(o, size, hi), n))
    bv.nbits = max(hi, 1)
    return bv


def replay_first(o, pa, sa, na, pb, sb, nb, proc: int):
    """sparse_vector_find_first_mismatch (:478-636) -> (found, idx)"""
    state = {"found": False, "mismatch": ID_MAX}

    def better(vec):
        f, midx = o.find_first(vec)
        if f and midx < state["mismatch"]:
            state["found"], state["mismatch"] = True, midx

    hi = max(sa, sb, 1)
    if proc == USE_NULL:                                              # :503-541
        if na is not None and nb is not None:
            better(o.op2(XOR, na, nb))
        else:
            if na is not None:
                better(o.op2(XOR, na, _ones_vec(o, sb, hi)))          # resize(sv2.size()); invert()
            if nb is not None:
                better(o.op2(XOR, nb, _ones_vec(o, sa, hi)))
    for i in range(max(len(pa), len(pb))):                            # :544-585 (planes of sv1 = P for two containers of one type)
        if not state["mismatch"]:
            break
        b1 = pa[i] if i < len(pa) else None
        b2 = pb[i] if i < len(pb) else None
        if b1 is None:
            if b2 is not None:
                better(b2)
            continue
        if b2 is None:
            better(b1)
            continue
        better(o.op2(XOR, b1, b2))
    return (True, int(state["mismatch"])) if state["found"] else (False, 0)


def oracle_case(o, case: dict) -> dict:
    vecs = _oracle_vecs(o, case)
    get = lambda col: ([vecs[k] if k is not None else None for k in col["planes"]], col["size"], vecs[col["nn"]] if col["nn"] is not None else None)
    a, b = get(case["a"]), get(case["b"])
    hi = case_size(case)
    out = {"size": hi}
    for name, proc in PROCS.items():
        m = replay_mismatch(o, *a, *b, proc)
        if m is None:
            r = {"count": None, "ids_sha": None}
        else:
            pos = ones_of(m)
            assert pos.size == 0 or int(pos.max()) < hi, "the replay left bits beyond the result's size"
            r = {"count": int(m.count()), "ids_sha": sha(pos.astype("<u8"))}
        f, idx = replay_first(o, *a, *b, proc)
        r["first"] = [bool(f), int(idx)]
        out[name] = r
    return out


# ---- the rules on rows' values and unpacked bits ----------------------------------------------------------------------------------
def _bits(case: dict, key, n: int) -> np.ndarray:
    out = np.zeros(n, bool)
    if key is not None:
        ids = case["vecs"][key][0]
        out[ids[ids < U(n)].astype(np.int64)] = True
    return out


def _values(case: dict, col: dict, n: int) -> np.ndarray:
    """the rows' values (plane i = bit i), zero beyond the planes' rows"""
    v = np.zeros(n, U)
    for i, k in enumerate(col["planes"]):
        if k is not None:
            v |= _bits(case, k, n).astype(U) << U(i)
    return v


def model_case(case: dict) -> dict:
    hi = case_size(case)
    sa, sb = case["a"]["size"], case["b"]["size"]
    lo = min(sa, sb)
    if case["values"] is not None:                                    # the values the planes were sliced from
        va, vb, null_a, null_b = case["values"]
        D = va != vb
        assert (_bits(case, case["a"]["nn"], hi) == ~null_a).all() and (_bits(case, case["b"]["nn"], hi) == ~null_b).all()
    else:
        D = _values(case, case["a"], hi) != _values(case, case["b"], hi)
    Na, Nb = _bits(case, case["a"]["nn"], hi), _bits(case, case["b"]["nn"], hi)
    has_a, has_b = case["a"]["nn"] is not None, case["b"]["nn"] is not None
    rows = np.arange(hi)
    out = {"size": hi}
    for name, proc in PROCS.items():
        M = D | ((rows >= lo) & (rows < hi))
        T = np.zeros(hi, bool)
        if proc == NO_NULL:
            if has_a or has_b:
                M = M & (Na | Nb)
        else:
            if has_a and has_b:
                M = M | (Na ^ Nb); T = Na ^ Nb
            elif has_a:
                M = M | ((rows < sa) & ~Na); T = Na ^ (rows < sb)
            elif has_b:
                M = M | ((rows < sb) & ~Nb); T = Nb ^ (rows < sa)
            else:
                M = None
        if not case["a"]["planes"] and not case["b"]["planes"] and M is not None:
            assert not M.any() and not T.any(), "a case without planes must be empty under the reference's rule too"
        pos = None if M is None else np.flatnonzero(M).astype("<u8")
        F = np.flatnonzero(D | T)
        out[name] = {"count": None if pos is None else int(pos.size), "ids_sha": None if pos is None else sha(pos),
                     "first": [bool(F.size), int(F[0]) if F.size else 0]}
    return out


# ---- the same operands on the device -----------------------------------------------------------------------------------------------
def device_vecs(bm, ctx, case: dict) -> dict:
    """key -> bvector: stored by content (NULL / FULL / GAP / bit-blocks), bit_keys as bit-blocks whatever they hold"""
    return {k: bm.bit_import_u32(ctx, case_words(case, k), k not in case["bit_keys"]) for k in case["vecs"]}


def device_scanners(bm, ctx, case: dict, vecs: dict | None = None):
    vecs = device_vecs(bm, ctx, case) if vecs is None else vecs
    mk = lambda col: bm.slice_scanner(ctx, [vecs[k] if k is not None else None for k in col["planes"]], size=col["size"],
                                      not_null=vecs[col["nn"]] if col["nn"] is not None else None)
    return mk(case["a"]), mk(case["b"])
