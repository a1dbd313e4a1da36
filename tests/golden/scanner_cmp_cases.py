"""Columns and expected values for the bit-sliced comparison search (bmx_slice_compare / bmx_slice_compare_signed and the
slice_scanner facade over them).  Pure NumPy: no device, no reference.

The expectation is ONE rule for both containers and every predicate: row i matches iff it is not NULL, i < size, and the
predicate holds for its value in plain integer arithmetic (int64 for the signed container, uint64 for the unsigned one;
a bound outside the array's type is compared as a Python int).  tests/test_scanner_model_host.py ties this rule to the
reference's results in golden_ref.json["scanner"].

A container keeps two invariants that the generators keep as well: a NULL row holds +0 (so the sign plane is a subset of the
not-NULL vector), and an operand that is shorter than the column reads as zeros past its end -- the value bit is 0, the sign
is "not negative", the row is NULL.  A row past the end of the not-NULL vector is therefore NULL AND holds 0."""
from __future__ import annotations

import functools

import numpy as np

B = 65536
NULL, FULL, BIT, GAP = 0, 1, 2, 3              # block kinds as the oracle's block table names them
I64_MIN, I64_MAX, U64_MAX = -(1 << 63), (1 << 63) - 1, (1 << 64) - 1
GT, GE, LT, LE, RANGE, EQ, ZERO, NONZERO = range(8)     # = BMX_CMP_*


# ---- the sign encoding (base_sparse_vector::s2u / u2s), on Python ints so that INT64_MIN and the 64-bit shift do not overflow ----
def s2u(v: int) -> int:
    v = int(v)
    assert I64_MIN <= v <= I64_MAX
    return v << 1 if v >= 0 else ((-(v + 1)) << 1) | 1


def u2s(u: int) -> int:
    u = int(u)
    assert 0 <= u <= U64_MAX
    return -(u >> 1) - 1 if u & 1 else u >> 1


def s2u_array(values: np.ndarray) -> np.ndarray:
    """int64 -> uint64, element-wise s2u: ~v == -(v + 1) needs no negation of INT64_MIN"""
    v = np.asarray(values, np.int64)
    neg = v < 0
    m = np.where(neg, ~v, v).astype(np.uint64)             # the magnitude: < 2^63
    return (m << np.uint64(1)) | neg.astype(np.uint64)


def u2s_array(u: np.ndarray) -> np.ndarray:
    u = np.asarray(u, np.uint64)
    m = (u >> np.uint64(1)).astype(np.int64)
    return np.where((u & np.uint64(1)) != 0, ~m, m)


def planes(values: np.ndarray, signed: bool, nplanes: int) -> list:
    """plane i of the column as a bool array, None where the plane is all zero (an absent plane).  Signed: plane 0 is the sign."""
    u = s2u_array(values) if signed else np.asarray(values, np.uint64)
    out = []
    for i in range(nplanes):
        bits = ((u >> np.uint64(i)) & np.uint64(1)) != 0 if i < 64 else np.zeros(u.size, bool)
        out.append(bits if bits.any() else None)
    assert nplanes >= 64 or not (u >> np.uint64(nplanes)).any(), "a value needs more planes than the column has"
    return out


# ---- the model ------------------------------------------------------------------------------------------------------------------
def _cmp(values: np.ndarray, op: str, bound: int) -> np.ndarray:
    info = np.iinfo(values.dtype)
    bound = int(bound)
    if bound > info.max:
        return np.full(values.size, op in ("lt", "le"))
    if bound < info.min:
        return np.full(values.size, op in ("gt", "ge"))
    b = values.dtype.type(bound)
    return {"gt": values > b, "ge": values >= b, "lt": values < b, "le": values <= b, "eq": values == b}[op]


def expect(pred: int, v0: int, v1: int, values: np.ndarray, valid, size: int) -> np.ndarray:
    """-> bool[size]: row i matches iff it is not NULL, i < size and the predicate holds for values[i].  Rows of [len(values),
    size) hold 0; with a not-NULL mask they are NULL as well.  A reversed range is swapped, as the reference does."""
    values = np.asarray(values)
    assert values.dtype in (np.int64, np.uint64)
    n = int(size)
    if values.size < n:
        values = np.concatenate([values, np.zeros(n - values.size, values.dtype)])
        if valid is not None:
            valid = np.concatenate([np.asarray(valid, bool), np.zeros(n - len(valid), bool)])
    values = values[:n]
    if pred == RANGE:
        lo, hi = (v0, v1) if v0 <= v1 else (v1, v0)
        r = _cmp(values, "ge", lo) & _cmp(values, "le", hi)
    elif pred == ZERO:
        r = _cmp(values, "eq", 0)
    elif pred == NONZERO:
        r = ~_cmp(values, "eq", 0)
    else:
        r = _cmp(values, {GT: "gt", GE: "ge", LT: "lt", LE: "le", EQ: "eq"}[pred], v0)
    if valid is not None:
        r = r & np.asarray(valid, bool)[:n]
    return r


def pack(bits: np.ndarray, nwords: int | None = None) -> np.ndarray:
    """bool rows -> uint32 words, bit i of the vector in bit (i & 31) of word i >> 5"""
    nw = (bits.size + 31) // 32 if nwords is None else nwords
    b = np.zeros(nw * 32, np.uint8)
    b[:bits.size] = bits
    return np.packbits(b, bitorder="little").view(np.uint32)


# ---- columns --------------------------------------------------------------------------------------------------------------------
class Column:
    """values: int64 / uint64 rows as the planes hold them; valid: bool mask or None (no not-NULL vector); size: the container's
    size(); nplanes: the length of the plane list (signed: sign + magnitude planes); lengths: operand -> bits uploaded, for
    "sign", "nn" and plane indices, where that is not len(values)"""

    def __init__(self, name, values, valid, size, nplanes, signed, lengths=None):
        self.name, self.values, self.valid, self.size, self.nplanes, self.signed = name, values, valid, int(size), nplanes, signed
        self.lengths = dict(lengths or {})
        assert valid is None or not values[~valid].any(), "a NULL row holds +0"

    def length(self, key) -> int:
        if self.signed and key == 0:
            key = "sign"
        return int(self.lengths.get(key, self.values.size))

    def operands(self):
        """-> (planes, nn): each plane / the not-NULL vector as (bool bits cut to the operand's length) or None"""
        pl = planes(self.values, self.signed, self.nplanes)
        pl = [None if p is None else p[:self.length(i)] for i, p in enumerate(pl)]
        nn = None if self.valid is None else self.valid[:self.length("nn")]
        return pl, nn

    def expect(self, pred, v0=0, v1=0, size=None) -> np.ndarray:
        return expect(pred, v0, v1, self.values, self.valid, self.size if size is None else size)

    def type_range(self):
        return (I64_MIN, I64_MAX) if self.signed else (0, U64_MAX)


def _runs(rng, n: int, mean: int) -> np.ndarray:
    """bool[n], constant over runs of about `mean` rows, alternating"""
    cuts = np.flatnonzero(rng.random(n) < 1.0 / mean)
    edge = np.zeros(n, np.int64)
    edge[cuts] = 1
    return (np.cumsum(edge) & 1) != 0


def _kind_bits(rng, kind: int, p_bit: float) -> np.ndarray:
    """one block of the given kind: NULL = zeros, FULL = ones, GAP = runs of about 900 rows, BIT = random at density p_bit"""
    if kind == NULL:
        return np.zeros(B, bool)
    if kind == FULL:
        return np.ones(B, bool)
    if kind == GAP:
        return _runs(rng, B, 900)
    return rng.random(B) < p_bit


KIND_OF_CODE = {0: NULL, 1: FULL, 2: GAP, 3: BIT}     # the grid's plan: block b -> code b & 3 / (b >> 2) & 3
GRID_BLOCKS = 16
GRID_ROWS = GRID_BLOCKS * B - 77
SPECIAL_BLOCK = 15                                   # BIT / BIT in the plan: fixed rows land here and break no FULL or NULL block
PARITY_BIT = 10                                      # the magnitude bit that every row of an odd block holds


def _grid_magnitudes(rng, n: int) -> np.ndarray:
    """uint64 magnitudes below 2^63: six random low bits (bit planes), bits 6..9 constant over runs of about 700 rows
    (GAP planes), bit 10 set in every row of the odd blocks (FULL and NULL plane blocks), about 0.05 % wide values over all the
    bits but bit 10 (sparse GAP blocks in the high planes)"""
    m = rng.integers(0, 64, n).astype(np.uint64)
    for bit in range(6, 10):
        m |= _runs(rng, n, 700).astype(np.uint64) << np.uint64(bit)
    wide = rng.random(n) < 0.0005
    w = rng.integers(0, 1 << 63, n, dtype=np.uint64)
    m = np.where(wide, w, m) & ~(np.uint64(1) << np.uint64(PARITY_BIT))
    odd = ((np.arange(n) >> 16) & 1) != 0
    return m | (odd.astype(np.uint64) << np.uint64(PARITY_BIT))


def _grid_masks(rng, n: int):
    """the planned (first, second) masks of the grid: block b gives `first` the kind b & 3 and `second` the kind (b >> 2) & 3"""
    first = np.concatenate([_kind_bits(rng, KIND_OF_CODE[b & 3], 0.5) for b in range(GRID_BLOCKS)])[:n]
    second = np.concatenate([_kind_bits(rng, KIND_OF_CODE[(b >> 2) & 3], 0.9) for b in range(GRID_BLOCKS)])[:n]
    return first, second


def _special_rows(n: int) -> np.ndarray:
    base = SPECIAL_BLOCK * B
    return np.array([base + 11, base + 12, base + 31, base + 32, base + 33, base + 30000, base + 40001, n - 1])


@functools.lru_cache(maxsize=None)
def kinds_signed64(with_null: bool = True, seed: int = 64001) -> Column:
    """16 blocks minus 77 rows of int64.  The sign plane follows the kind plan b & 3, the not-NULL vector (b >> 2) & 3; with a
    not-NULL vector the sign is cut to it (a NULL row holds +0), without one the sign kinds are free: a FULL sign block over
    non-trivial magnitudes.  64 planes (sign + 63) with NULLs, 65 (the last one absent) without."""
    rng = np.random.default_rng(seed)
    n = GRID_ROWS
    sign, valid = _grid_masks(rng, n)
    m = _grid_magnitudes(rng, n).astype(np.int64)
    v = np.where(sign, ~m, m)
    rows = _special_rows(n)
    v[rows] = [I64_MIN, I64_MAX, -1, 0, 1, I64_MIN + 1, -2, 5]
    valid[rows] = True
    if with_null:
        v[~valid] = 0
    return Column("kinds_signed64" if with_null else "kinds_signed64_nonull", v, valid if with_null else None, n,
                  64 if with_null else 65, True)


@functools.lru_cache(maxsize=None)
def kinds_unsigned64(with_null: bool = True, seed: int = 64002) -> Column:
    """the same grid for the unsigned container over 64 planes: plane 63 follows the kind plan b & 3"""
    rng = np.random.default_rng(seed)
    n = GRID_ROWS
    top, valid = _grid_masks(rng, n)
    top_bit = np.uint64(1) << np.uint64(63)
    v = (_grid_magnitudes(rng, n) & ~top_bit) | (top.astype(np.uint64) << np.uint64(63))
    rows = _special_rows(n)
    v[rows] = np.array([U64_MAX, 1 << 63, (1 << 63) - 1, 0, 1, U64_MAX - 1, 2, 5], np.uint64)
    valid[rows] = True
    if with_null:
        v[~valid] = 0
    return Column("kinds_unsigned64" if with_null else "kinds_unsigned64_nonull", v, valid if with_null else None, n, 64, False)


NARROW_ROWS = 3 * B + 999
NARROW_KINDS = ("plane4_absent", "sign_absent", "sign_only", "no_planes")


@functools.lru_cache(maxsize=None)
def narrow_signed(kind: str, with_null: bool = True, seed: int = 64003) -> Column:
    """3 blocks + 999 rows of a signed container: 11 planes with plane 4 absent / no sign plane (values >= 0) / nothing but the
    sign plane (values 0 and -1) / no planes at all (every value 0)"""
    rng = np.random.default_rng(seed + NARROW_KINDS.index(kind))
    n = NARROW_ROWS
    valid = rng.random(n) < 0.9
    valid[[0, n - 1]] = True
    if kind == "plane4_absent":
        m = rng.integers(0, 1 << 10, n) & ~(1 << 3)                     # magnitude bit 3 = plane 4
        v, nplanes = np.where(rng.random(n) < 0.5, ~m, m).astype(np.int64), 11
        v[70000:71000] = 0; v[71000:72000] = -1
    elif kind == "sign_absent":
        v, nplanes = rng.integers(0, 1 << 10, n).astype(np.int64), 11
    elif kind == "sign_only":
        v, nplanes = -(rng.random(n) < 0.5).astype(np.int64), 1
    else:
        v, nplanes = np.zeros(n, np.int64), 0
    if with_null:
        v[~valid] = 0
    return Column("narrow_%s%s" % (kind, "" if with_null else "_nonull"), v, valid if with_null else None, n, nplanes, True)


SHORT_ROWS = 5 * B + 4321


@functools.lru_cache(maxsize=None)
def short_operands(signed: bool = True, with_null: bool = True, seed: int = 64004) -> Column:
    """5 blocks + 4,321 rows, 12 planes.  Plane 0 (the sign of the signed form) is uploaded over its first 2 blocks only, the
    not-NULL vector over 3, plane 5 over 1: past an operand's end the rows read as bit 0 / not negative / NULL, and the values
    the model sees are the ones the cut planes spell."""
    rng = np.random.default_rng(seed)
    n = SHORT_ROWS
    lengths = {("sign" if signed else 0): 2 * B, "nn": 3 * B, 5: B}
    u = rng.integers(0, 1 << 12, n).astype(np.uint64)
    idx = np.arange(n)
    u[idx >= 2 * B] &= ~np.uint64(1)
    u[idx >= B] &= ~(np.uint64(1) << np.uint64(5))
    valid = rng.random(n) < 0.9
    valid[idx >= 3 * B] = False
    if with_null:
        u[~valid] = 0
    else:
        del lengths["nn"]
    v = u2s_array(u) if signed else u
    return Column("short_operands_%s%s" % ("signed" if signed else "unsigned", "" if with_null else "_nonull"), v,
                  valid if with_null else None, n, 12, signed, lengths)


def all_columns() -> dict:
    """name -> zero-argument constructor of every column of the comparison tests"""
    out = {}
    for wn in (True, False):
        for f in (kinds_signed64, kinds_unsigned64):
            out[f(wn).name] = functools.partial(f, wn)
        for k in NARROW_KINDS:
            out[narrow_signed(k, wn).name] = functools.partial(narrow_signed, k, wn)
        for sg in (True, False):
            out[short_operands(sg, wn).name] = functools.partial(short_operands, sg, wn)
    return out


# ---- bounds and ranges of a column ----------------------------------------------------------------------------------------------
def present_values(col: Column, k: int = 6) -> list:
    """k values the column holds, spread over its sorted distinct not-NULL values (the extremes among them)"""
    vals = col.values[:col.size] if col.valid is None else col.values[:col.size][col.valid[:col.size]]
    d = np.unique(vals)
    pick = d[np.unique(np.linspace(0, d.size - 1, min(k, d.size)).astype(np.int64))] if d.size else d
    return [int(x) for x in pick]


def max_magnitude(col: Column) -> int:
    """the largest magnitude the planes can hold"""
    nmag = col.nplanes - 1 if col.signed else col.nplanes
    return (1 << min(max(nmag, 0), 63 if col.signed else 64)) - 1


def bounds(col: Column) -> list:
    """the extremes of the type; 0, +-1, +-2; six present values and each of them +-1; the largest magnitude the planes hold
    and that + 1 (signed: their negatives too); +-2^40 on the narrow columns (a bit above every plane on both sides of zero).
    Whatever falls outside the type is left out: the entry cannot take it."""
    lo, hi = col.type_range()
    b = [lo, hi, 0, 1, 2, -1, -2]
    for p in present_values(col):
        b += [p - 1, p, p + 1]
    mm = max_magnitude(col)
    b += [mm, mm + 1, -mm, -(mm + 1), -(mm + 2)]          # (-(mm + 1) is the most negative value mm planes spell)
    if col.nplanes < 41:
        b += [1 << 40, -(1 << 40)]
    return sorted({x for x in b if lo <= x <= hi})


def ranges(col: Column) -> list:
    """both bounds negative, both non-negative, straddling zero, reversed, equal; [MIN, MAX], [MIN, -1], [0, MAX], [-1, 0];
    three pairs of present values.  For the unsigned container the negative ones fall away."""
    lo, hi = col.type_range()
    p = present_values(col)
    r = [(-50, -10), (10, 50), (-5, 5), (40, -40), (90, 10), (3, 3), (-1, -1), (0, 0), (lo, hi), (lo, -1), (0, hi), (-1, 0)]
    if len(p) >= 2:
        r += [(p[0], p[-1]), (p[1], p[-2]), (p[len(p) // 2], p[-1])]
    return [x for x in dict.fromkeys(r) if lo <= x[0] <= hi and lo <= x[1] <= hi]
