"""The operands of remap_ref.json (bm::set2set_11_transform<SV>::remap, src/bmsparsevec_algo.h:2096-2205) and the model the tests
hold the device against.  Shared by make_remap_golden.py and the tests; every operand comes from fixed seeds and is held as the
ascending positions of its ones.

A case is {"vecs": key -> (positions, nbits), "planes": [key or None, ...], "size": rows, "nn": key of the not-NULL vector or None,
"sel": key of the selector bv_in or None (every row), "values": (values, is_null) the planes were sliced from or None}: the same key
is the same vector (one handle on the device).

  model   rows  = ones(bv_in & not_null & [0, size))          the rows remap enumerates (:2134-2144), cut at size
          vals  = values[rows]                                plane i = bit i, zero beyond a plane's rows
          image = unique(vals)                                bv_out; a value at or beyond 2^36 (IMAGE_LIMIT: the 2^20 blocks of a
                                                              device vector) has no image there: BMX_ERR_RANGE

The reference shim exports no set2set, so make_remap_golden.py anchors the model in the reference through the calls it does export
(anchor_case): only cases built from values ("values" is not None), unsigned, at most 32 planes, a few hundred distinct image
values at the most."""
from __future__ import annotations

import functools

import numpy as np

from import_cases import sha  # noqa: F401
from kleene_cases import K_BIT, K_FULL, K_GAP, K_NULL, _mixed, _vec  # noqa: F401
from rankc_cases import _cat, ones_of, oracle_vec, words_of  # noqa: F401

B = 65536
U = np.uint64
AND = 0
CMP_EQ = 5
IMAGE_LIMIT = 1 << 36
SWEEP_COUNTS = [min(c, B) for k in range(6, 17) for c in ((1 << k) - 1, 1 << k, (1 << k) + 1)]     # 33 columns


def _case(vecs, planes, size, nn=None, sel=None, values=None, bit_keys=()):
    return {"vecs": vecs, "planes": list(planes), "size": int(size), "nn": nn, "sel": sel, "values": values, "bit_keys": frozenset(bit_keys)}


def _cut(v, nbits):
    ids, _ = v
    return ids[ids < U(nbits)], int(nbits)


def _slice_planes(values: np.ndarray, nplanes: int, rows: int, prefix: str = "p") -> dict:
    v = values.astype(U)
    return {"%s%d" % (prefix, i): (np.flatnonzero((v >> U(i)) & U(1)).astype(U), rows) for i in range(nplanes)}


def _from_values(values, is_null, sel_ids, nplanes=32, with_nn=True, sel_nbits=None):
    """a column sliced from values (NULL rows hold 0) with a selector"""
    rows = int(values.size)
    values = values.copy()
    values[is_null] = 0
    vecs = _slice_planes(values, nplanes, rows)
    if with_nn:
        vecs["nn"] = (np.flatnonzero(~is_null).astype(U), rows)
    if sel_ids is not None:
        vecs["sel"] = (np.asarray(sel_ids, U), int(sel_nbits or rows))
    return _case(vecs, ["p%d" % i for i in range(nplanes)], rows, "nn" if with_nn else None, "sel" if sel_ids is not None else None,
                 values=(values, is_null))


def _sweep():
    """33 columns whose selected counts bracket every power of two from 64 to 65536; the 65536 columns are FULL selector blocks"""
    nb = len(SWEEP_COUNTS)
    rows = nb * B
    rng = np.random.default_rng(77)
    values = rng.integers(0, 1 << 32, rows, dtype=np.uint64)
    sel = [c * B + (np.arange(B) if n == B else np.sort(rng.choice(B, size=n, replace=False))) for c, n in enumerate(SWEEP_COUNTS)]
    return _from_values(values, np.zeros(rows, bool), np.concatenate(sel).astype(U), with_nn=False)


@functools.lru_cache(maxsize=None)
def cases():
    c = {}
    # ---- block-kind grids over 15 columns, size inside the last one: selector x not-NULL (every pair but NULL / NULL), then
    #      selector x plane 0 with plane 1 carrying the transposed plan and no not-NULL vector
    gs = 14 * B + 1000
    q = [k + 1 for k in range(15)]
    g = {"sel": _vec([x & 3 for x in q], 701, gs), "nn": _vec([x >> 2 for x in q], 702, gs),
         "p0": _vec([(x + 1) & 3 for x in q], 703, gs), "p1": _vec([(x >> 1) & 3 for x in q], 704, gs), "p2": _cut(_mixed(705, 15), gs)}
    c["grid"] = _case(g, ["p0", "p1", "p2"], gs, "nn", "sel")
    g2 = {"sel": g["sel"], "p0": _vec([x >> 2 for x in q], 706, gs), "p1": _vec([x & 3 for x in q], 707, gs)}
    c["grid_planes"] = _case(g2, ["p0", "p1"], gs, None, "sel")
    # ---- the selected-rows sweep
    c["sweep"] = _sweep()
    # ---- plane counts
    ps = 2 * B + 300
    psel = _cut(_mixed(710, 3), ps)
    c["planes_0"] = _case({"sel": psel, "nn": _cut(_mixed(711, 3), ps)}, [], ps, "nn", "sel")
    c["planes_0_nothing_selected"] = _case({"sel": (np.zeros(0, U), ps)}, [], ps, None, "sel")
    c["planes_1"] = _case({"sel": psel, "p0": _cut(_mixed(712, 3), ps)}, ["p0"], ps, None, "sel")
    for n in (33, 64):
        pv = {"p%d" % i: _cut(_mixed(720 + 100 * n + i, 3), ps) for i in range(n)}
        pv.update(sel=_cut(_vec([K_GAP, K_GAP, K_GAP], 713), ps), nn=_cut(_mixed(714, 3), ps))
        c["planes_%d" % n] = _case(pv, ["p%d" % i for i in range(n)], ps, "nn", "sel")
    # 64 planes whose image fits a device vector: planes 36..63 hold ones only in NULL rows
    hv = dict(c["planes_64"]["vecs"])
    for i in range(36, 64):
        hv["p%d" % i] = (np.setdiff1d(hv["p%d" % i][0], hv["nn"][0]).astype(U), ps)
    c["planes_64_image"] = _case(hv, ["p%d" % i for i in range(64)], ps, "nn", "sel")
    av = {"p%d" % i: _cut(_mixed(730 + i, 3), ps) for i in (0, 1, 3, 5)}
    av["sel"] = psel
    c["absent_planes"] = _case(av, ["p0", "p1", None, "p3", None, "p5"], ps, None, "sel")
    ss = 4 * B + 10
    sv = {"p0": _cut(_mixed(740, 5), ss), "p1": _cut(_mixed(741, 3), 3 * B - 5), "p2": _cut(_mixed(742, 5), ss), "sel": _cut(_mixed(743, 5), ss)}
    c["short_plane"] = _case(sv, ["p0", "p1", "p2"], ss, None, "sel")
    # ---- selector length: longer than the column (bits beyond size in the tail block and in later blocks), shorter, none
    ls = 2 * B + 5000
    lv = {"p%d" % i: _cut(_mixed(750 + i, 3), ls) for i in range(4)}
    lv.update(nn=_cut(_mixed(755, 3), ls), long=_vec([K_BIT, K_GAP, K_FULL, K_BIT, K_FULL, K_GAP], 756), short=_cut(_mixed(757, 2), B + 77))
    c["sel_longer"] = _case(lv, ["p0", "p1", "p2", "p3"], ls, "nn", "long")
    c["sel_longer_no_nn"] = _case(lv, ["p0", "p1", "p2", "p3"], ls, None, "long")
    c["sel_shorter"] = _case(lv, ["p0", "p1", "p2", "p3"], ls, "nn", "short")
    c["sel_none"] = _case(lv, ["p0", "p1", "p2", "p3"], ls, "nn", None)
    c["sel_none_no_nn"] = _case(lv, ["p0", "p1", "p2", "p3"], ls, None, None)
    c["size_zero"] = _case({"p0": (np.zeros(0, U), 5), "sel": (np.array([0, 3], U), 5)}, ["p0"], 0, None, "sel")
    # ---- values: M:1, value 0 with and without a not-NULL vector, the largest 32-bit value
    rows = 3 * B - 1000
    rng = np.random.default_rng(780)
    sel_ids = np.flatnonzero(rng.random(rows) < 0.2)
    m1 = rng.integers(0, 50, rows, dtype=np.uint64)
    c["m_to_1"] = _from_values(m1, rng.random(rows) < 0.05, sel_ids)
    zr = rng.integers(0, 300, rows, dtype=np.uint64)
    zr[rng.random(rows) < 0.3] = 0
    c["zero_with_nn"] = _from_values(zr, rng.random(rows) < 0.1, sel_ids)
    c["zero_without_nn"] = _from_values(zr, rng.random(rows) < 0.1, sel_ids, with_nn=False)
    only0 = np.zeros(B + 9, U)
    c["only_zero_with_nn_all_null"] = _from_values(only0, np.ones(B + 9, bool), np.arange(0, B + 9, 3))
    c["only_zero_without_nn"] = _from_values(only0, np.zeros(B + 9, bool), np.arange(0, B + 9, 3), with_nn=False)
    mx = rng.integers(0, 200, 2 * B, dtype=np.uint64)
    mx[[5, B + 17]] = (1 << 32) - 1
    mx[[6, 77]] = 1 << 31
    c["max_u32"] = _from_values(mx, np.zeros(2 * B, bool), np.concatenate([[5, 6, 77, B + 17], np.arange(100, 2 * B, 97)]))
    c["values_32"] = _from_values(rng.integers(0, 1 << 32, rows, dtype=np.uint64), rng.random(rows) < 0.05, sel_ids)
    # ---- width 8: a value of 36 bits (a high output block) among small ones, 40 planes
    w8 = rng.integers(0, 1000, B + 500, dtype=np.uint64)
    w8[[4, 66000]] = (1 << 35) + 12345
    w8[10] = (1 << 36) - 1
    c["wide_36"] = _from_values(w8, np.zeros(B + 500, bool), np.arange(0, B + 500, 2), nplanes=40)
    return c


def anchored(case: dict) -> bool:
    return case["values"] is not None and len(case["planes"]) <= 32 and model_case(case)["image"].size <= 400


# ---- the model -----------------------------------------------------------------------------------------------------------------------
def _bits(case: dict, key, n: int, absent: bool) -> np.ndarray:
    if key is None:
        return np.full(n, absent, bool)
    out = np.zeros(n, bool)
    ids = case["vecs"][key][0]
    out[ids[ids < U(n)].astype(np.int64)] = True
    return out


def model_case(case: dict) -> dict:
    """-> rows (uint64), values (uint64, by row), image (uint64, ascending)"""
    n = case["size"]
    S = _bits(case, case["sel"], n, True) & _bits(case, case["nn"], n, True)
    rows = np.flatnonzero(S).astype(U)
    vals = np.zeros(rows.size, U)
    for i, k in enumerate(case["planes"]):
        if k is not None:
            vals |= _bits(case, k, n, False)[rows.astype(np.int64)].astype(U) << U(i)
    if case["values"] is not None:
        assert np.array_equal(vals, case["values"][0][rows.astype(np.int64)].astype(U)), "the planes do not spell the values"
    return {"rows": rows, "values": vals, "image": np.unique(vals)}


def record(m: dict) -> dict:
    img = m["image"]
    return {"n_rows": int(m["rows"].size), "rows_sha": sha(m["rows"].astype("<u8")), "values_sha": sha(m["values"].astype("<u8")),
            "image_count": int(img.size), "image_sha": sha(img.astype("<u8")), "image_max": int(img.max()) if img.size else None}


# ---- the model against the reference (generator only) -------------------------------------------------------------------------------
def anchor_case(R, case: dict) -> dict:
    """the planes and the not-NULL vector are those of the reference's container; every image value is found by the reference's
    scanner among the selected rows, and the per-value counts add up to count(sel & not_null): every selected row is accounted
    for and no value is invented"""
    values, is_null = case["values"]
    n = case["size"]
    has_nn = case["nn"] is not None
    sv = R.sparse_vector(values.astype(np.uint32), is_null.astype(np.uint8) if has_nn else None)   # (NULL rows hold 0 either way)
    assert sv.size() == n
    for i, k in enumerate(case["planes"]):
        s = sv.slice(i)
        got = ones_of(s) if s is not None else np.zeros(0, U)
        assert np.array_equal(got, case["vecs"][k][0]), ("plane", i)
    nn = sv.not_null()
    assert (nn is not None) == has_nn
    if has_nn:
        assert np.array_equal(ones_of(nn), case["vecs"][case["nn"]][0])
    m = model_case(case)
    sel_ids = case["vecs"][case["sel"]][0] if case["sel"] is not None else np.arange(n, dtype=U)
    assert sel_ids.size == 0 or int(sel_ids.max()) < n, "an anchored selector stays inside the column"
    sel = oracle_vec(R, sel_ids, max(n, 1))
    if has_nn:
        sel = R.op2(AND, sel, nn)
    total = 0
    for v in m["image"]:
        hit = int(R.op2(AND, sv.compare(CMP_EQ, int(v)), sel).count())
        assert hit > 0, ("image value without a row", int(v))
        total += hit
    assert total == int(sel.count()) == m["rows"].size
    return {"distinct": int(m["image"].size), "rows": total}


# ---- the same operands on the device -------------------------------------------------------------------------------------------------
def case_words(case: dict, key: str) -> np.ndarray:
    ids, nbits = case["vecs"][key]
    return words_of(ids, max(nbits, 1))


def device_vecs(bm, ctx, case: dict) -> dict:
    return {k: bm.bit_import_u32(ctx, case_words(case, k), k not in case["bit_keys"]) for k in case["vecs"]}


def device_scanner(bm, ctx, case: dict, vecs: dict | None = None):
    """-> (slice_scanner, selector bvector or None, vecs)"""
    vecs = device_vecs(bm, ctx, case) if vecs is None else vecs
    sc = bm.slice_scanner(ctx, [vecs[k] if k is not None else None for k in case["planes"]], size=case["size"],
                          not_null=vecs[case["nn"]] if case["nn"] is not None else None)
    return sc, (vecs[case["sel"]] if case["sel"] is not None else None), vecs
