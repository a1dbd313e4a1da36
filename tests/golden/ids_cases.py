"""Constructed cases for vectors built from id lists (bvector::set(ids, n, sort_order) on an empty vector; bmx_kernels13.h and
k_scan_layout; tests/test_ids_host.py, tests/test_gpu_ids.py): every border of the import is met on purpose, each case with its
answer in closed form.

A case is a spec, not a list: an ordered sequence of segments (block, offsets, repeat).  The id list is the concatenation of
np.repeat(block * 65536 + offsets, repeat) over the segments, then put into the case's order (as built, reversed, permuted, or
rotated around one descent).  The answer never looks at the ids: expected_table() takes the union of the offsets per block and
writes the table in the layout the device writes.  plan() restates, as integers, what ids_import_t (bmx.hip) decides for a list;
the host test uses it to prove that a case meets the border its name claims.

A FULL block costs 65,536 ids and a bit-block under optimize 638, so the grids that need many touched blocks (I4) keep most of
them GAP and place the FULL and bit-blocks where the layout scan has its borders: every case but the few named in BIG stays at
or below PORT_LIMIT ids, which is what the oracle port checks id by id.

The constants restate the source; the host test reads them back from the headers and bmx.hip.  No GPU, no oracle: pure NumPy."""
import numpy as np

from and_fold_cases import B, BW, NULL, FULL, BIT, GAP, MAX_GAP_LEN, block_of, block_of_ends, gap_words, kind_of, words_of
from import_cases import canonical, record  # noqa: F401  (record: what the fixtures hold)

IDS_CHUNK = 4096            # bmx_kernels13.h: ids per workgroup of k_ids_scan / k_ids_starts
TBL_PER = 4096              # entries per workgroup of the k_tbl_* scan
IDS_LDS_BLOCKS = 16384      # shards of at most this many blocks take the LDS histogram / scatter
LGRID_IDS = 4096            # bmx.hip ids_import_t: lgrid = min(ceil(n / 4096), 512)
LGRID_MAX = 512
IMAGE_BATCH = 512           # ids_image: ids per pass of a wave
SCAN_LAYOUT_PER = 8         # bmx_kernels.h k_scan_layout: entries per lane; a wave 64 x 8, a pass 1,024 x 8
LAYOUT_WAVE = 64 * SCAN_LAYOUT_PER
LAYOUT_PASS = 1024 * SCAN_LAYOUT_PER
GAP_RUNS_END = 1276         # k_ids_stats: runs < 1276 -> GAP
IDS_MAX_BLOCKS = 1 << 20
ALL = 0xFFFFFFFF
PORT_LIMIT = 300_000        # cases up to this many ids are compared with the oracle port id by id
LARGE = 1_000_000           # beyond: one width, both sources, BM_UNKNOWN only on the GPU

LEVEL_LENS = (124, 125, 252, 253, 508, 509, 1275, 1276, 1277)
RUN_LENS = tuple(range(2, 18)) + LEVEL_LENS
BIT_POS = (0, 1, 31, 32, 127, 128, 8191, 8192, 65534, 65535)
IDS_PER_BLOCK = (1, 2, 63, 64, 65, 511, 512, 513, 1023, 1024, 1025)
CHANGE_AT = (1, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097)
DESCENT_AT = (1, 64, 256, 4095, 4096, 4097)
N_SORTED = (1, 255, 256, 257, 4095, 4096, 4097, 8191, 8192, 8193)
TOUCHED = (3, 4, 5, 63, 64, 65, 511, 512, 513, 8191, 8192, 8193)
LDS_NBL = (16383, 16384, 16385)


def seg(block, offs, rep=1):
    offs = np.asarray(offs, np.int64).reshape(-1)
    assert offs.size and 0 <= offs.min() and offs.max() < B and rep >= 1 and 0 <= block < IDS_MAX_BLOCKS
    return (int(block), offs, int(rep))


def expand(spec):
    """the id list of a spec, as built (uint64)"""
    if not spec: return np.zeros(0, np.uint64)
    return np.concatenate([np.repeat((np.uint64(b * B) + o.astype(np.uint64)), r) for b, o, r in spec])


def spec_len(spec):
    return sum(o.size * r for _, o, r in spec)


def spec_max(spec):
    return max(b * B + int(o.max()) for b, o, _ in spec) if spec else -1


def spec_from_ids(ids):
    """a spec whose expansion is the list: one segment per stretch of one block's ids"""
    ids = np.asarray(ids, np.uint64)
    if not ids.size: return []
    blk = (ids >> np.uint64(16)).astype(np.int64)
    cut = np.flatnonzero(blk[1:] != blk[:-1]) + 1
    return [seg(blk[a], (ids[a:b] & np.uint64(0xFFFF)).astype(np.int64)) for a, b in zip(np.concatenate([[0], cut]), np.concatenate([cut, [ids.size]]))]


def block_offsets(spec):
    """block -> the sorted distinct offsets of its ids"""
    d = {}
    for b, o, _ in spec: d.setdefault(b, []).append(o)
    return {b: np.unique(np.concatenate(d[b])) for b in sorted(d)}


def window_of(nbits, window):
    """shard_window (bmx.hip): nb_to clamped to the vector -> (nb_from, nb_to, bits of the shard), None where nb_from > nb_to"""
    nblocks = (nbits + B - 1) // B
    f, t = (0, ALL) if window is None else window
    t = min(t, nblocks)
    if f > t: return None
    return f, t, max(min(nbits, t * B) - f * B, 0)


def expected_table(spec, nbits=0, optimize=False, window=None):
    """-> (nbits_out, kinds, offs, bit_slab, gap_slab) of the vector (or of its blocks [nb_from, nb_to)) the spec's ids build:
    without optimize every touched block a bit-block; with it one run FULL, up to MAX_GAP_LEN runs GAP, else a bit-block.
    Bit-blocks by ordinal; GAP blocks from 16-byte boundaries, 0xFFFF padding (k_ids_emit, gap_close)"""
    size = max(int(nbits), spec_max(spec) + 1)
    w = window_of(size, window)
    if w is None: raise ValueError("nb_from > nb_to")
    f, t, bits = w
    kinds, offs = np.zeros(t - f, np.uint8), np.zeros(t - f, np.uint32)
    bit_parts, gap_parts, gpos = [], [], 0
    for blk, u in block_offsets(spec).items():
        if not f <= blk < t: continue
        b = np.zeros(B, bool); b[u] = True
        k = kind_of(b) if optimize else BIT
        assert k != NULL
        kinds[blk - f] = k
        if k == BIT:
            offs[blk - f] = len(bit_parts); bit_parts.append(words_of(b))
        elif k == GAP:
            g = gap_words(b)
            p = np.full((g.size + 7) & ~7, 0xFFFF, np.uint16); p[:g.size] = g
            offs[blk - f] = gpos; gpos += p.size; gap_parts.append(p)
    bit_slab = np.concatenate(bit_parts) if bit_parts else np.zeros(0, np.uint32)
    gap_slab = np.concatenate(gap_parts) if gap_parts else np.zeros(0, np.uint16)
    return bits, kinds, offs, bit_slab, gap_slab


def mask_levels(kinds, offs, gaps):
    """the GAP slab with the level bits of every header cleared (an allocator detail)"""
    g = np.array(gaps, np.uint16, copy=True)
    g[np.asarray(offs)[np.asarray(kinds) == GAP]] &= 0xFFF9
    return g


def plan(ids, nbits=0, window=None):
    """what ids_import_t decides for this list, and where the list meets the kernels' borders"""
    ids = np.asarray(ids, np.uint64)
    n = int(ids.size)
    p = {"n": n, "nchunks": (n + IDS_CHUNK - 1) // IDS_CHUNK}
    if not n:
        p.update(sorted=True, size=int(nbits)); return p
    blk = (ids >> np.uint64(16)).astype(np.int64)
    down = np.flatnonzero(ids[1:] < ids[:-1]) + 1
    change = np.flatnonzero(blk[1:] != blk[:-1]) + 1
    mx = int(ids.max())
    size = max(int(nbits), mx + 1)
    f, t, bits = window_of(size, window)
    nbl = t - f
    inside = np.unique(blk[(blk >= f) & (blk < t)])
    p.update(sorted=down.size == 0, descents=down, changes=change, block_runs=int(change.size) + 1, distinct_blocks=int(np.unique(blk).size),
             max_id=mx, size=size, nb_from=f, nb_to=t, nbl=nbl, bits=bits, touched=int(inside.size))
    starts = np.bincount(np.concatenate([[0], change]) // IDS_CHUNK, minlength=p["nchunks"])
    p["chunk_starts"] = starts
    if p["sorted"]:
        p.update(nparts=(p["nchunks"] + TBL_PER - 1) // TBL_PER, cap=min(n, (mx >> 16) + 1))
    else:
        lgrid = min((n + LGRID_IDS - 1) // LGRID_IDS, LGRID_MAX)
        p.update(nparts=(nbl + TBL_PER - 1) // TBL_PER, cap=min(n, nbl), lds=nbl <= IDS_LDS_BLOCKS, lds_bytes=nbl * 4, lgrid=lgrid,
                 per=(n + lgrid - 1) // lgrid)
    return p


# ---------------------------------------------------------------------------------------------------------------------
# orders
# ---------------------------------------------------------------------------------------------------------------------
def rotation(L, p):
    """s such that L[s:s+p] + L[:s] + L[s+p:] (L non-decreasing) has its only descent at index p and holds one block in two
    separate runs; None where the list has no such s"""
    n = L.size
    if n < p + 2: return None
    blk = L >> np.uint64(16)
    s = np.arange(1, n - p + 1)
    last = blk[s + p - 1]                                            # the block in front of the descent
    again = np.zeros(s.size, bool)
    again[:-1] = blk[s[:-1] + p] == last[:-1]                        # ... goes on behind the moved head
    twice = np.zeros(s.size, bool)
    twice[1:] = blk[s[1:] - 1] == blk[s[1:]]                         # or: the cut falls inside a block (needs s >= 2)
    ok = (last > blk[0]) & (again | (twice & (blk[s] > blk[0])))
    hit = np.flatnonzero(ok)
    return int(s[hit[0]]) if hit.size else None


class Case:
    def __init__(self, name, spec, nbits=0, order=None, flavour="avx2", twin=None, **claims):
        self.name, self.spec, self.nbits, self.order, self.flavour, self.twin, self.claims = name, spec, int(nbits), order, flavour, twin, claims
        self.sorted = self.claims.pop("sorted", order is None)         # what the list is, whatever flag a call passes
        self.n = spec_len(spec)
        self.grid = name.split("/")[0]
        self._exp = {}

    def __repr__(self): return self.name

    def ids(self):
        L = expand(self.spec)
        o = self.order
        if o is None: return L
        if o == "rev": return L[::-1].copy()
        if o == "perm": return L[np.random.default_rng(L.size).permutation(L.size)]
        _, p, s = o
        return np.concatenate([L[s:s + p], L[:s], L[s + p:]])

    def max_id(self): return spec_max(self.spec)

    def widths(self): return (4, 8) if self.max_id() < (1 << 32) else (8,)

    def size(self): return max(self.nbits, self.max_id() + 1)

    def uniq(self):
        return np.concatenate([np.uint64(b * B) + u.astype(np.uint64) for b, u in block_offsets(self.spec).items()] or [np.zeros(0, np.uint64)])

    def expected(self, optimize, window=None):
        """cached per spec: the orders of one list share it (and must not change it)"""
        cache = _SPEC_CACHE.setdefault(id(self.spec), {})
        key = (self.nbits, bool(optimize), window)
        if key not in cache: cache[key] = expected_table(self.spec, self.nbits, optimize, window)
        return cache[key]

    def shrunk(self):
        """the twin of a large case: the same segments with smaller repeat counts"""
        return Case(self.name + "/twin", [(b, o, max(1, r // 64)) for b, o, r in self.spec], self.nbits, self.order if self.order in (None, "rev") else None)


_SPEC_CACHE = {}


# ---------------------------------------------------------------------------------------------------------------------
# I1: sorted positions
# ---------------------------------------------------------------------------------------------------------------------
def two_blocks(n, p, b0=2, b1=5):
    """n ascending ids, the first p in block b0 and the rest in block b1"""
    s = []
    if p: s.append(seg(b0, 7 + 3 * np.arange(p)))
    if n - p: s.append(seg(b1, 11 + 5 * np.arange(n - p)))
    return s


def _two_parts(extra):
    """2^24 ascending ids: blocks 1 and 2 full many times over, block 3 opening ten ids into chunk 4,095; then `extra`"""
    head = [seg(1, np.arange(B), 100), seg(2, np.arange(61450), 156), seg(2, np.arange(61450, B), 155)]
    assert spec_len(head) == 4095 * IDS_CHUNK + 10
    return head + [seg(3, 3 * np.arange(IDS_CHUNK - 10))] + extra


def grid_i1():
    c = []
    for n in N_SORTED:
        c.append(Case("I1/n_%d" % n, two_blocks(n, n // 2), n=n))
    n = 8193
    for p in CHANGE_AT + (n - 1,):
        c.append(Case("I1/change_at_%d" % p, two_blocks(n, p), change=p))
    c.append(Case("I1/every_id_a_new_block", [seg(i, [(i * 37) % B]) for i in range(4097)], cap_is_n=True))
    c.append(Case("I1/block_of_70000", [seg(1, [3, 9, 27, 81, 243]), seg(3, 1 + np.arange(35000), 2), seg(6, [0, 5, 6, 7, 65535])],
                  zero_start_chunks=16))
    c.append(Case("I1/last_chunk_one_id", two_blocks(4097, 4096, 2, 9), change=4096))
    c.append(Case("I1/equal_over_chunk_border", [seg(2, 10 + 2 * np.arange(2731), 3), seg(4, [1, 2, 3])], equal_at=(4096, 8192)))
    c.append(Case("I1/equal_then_change_at_8192", [seg(2, [0]), seg(2, 1 + np.arange(4095), 2), seg(2, [5000]), seg(7, [9], 3)],
                  equal_at=(4096,), change=8192))
    c.append(Case("I1/two_parts_below", _two_parts([]), nparts=1, change_chunks=(4095,)))
    c.append(Case("I1/two_parts_first_entry", _two_parts([seg(7, [B - 1])]), nparts=2, change_chunks=(4095, 4096)))
    c.append(Case("I1/two_parts_tail", _two_parts([seg(5, 2 * np.arange(100)), seg(6, np.arange(8000)), seg(9, [0, 1, 40000])]), nparts=2,
                  change_chunks=(4095, 4096, 4097)))
    return c


# ---------------------------------------------------------------------------------------------------------------------
# I2: unsorted positions
# ---------------------------------------------------------------------------------------------------------------------
def _wg512(n):
    """n ids for 512 workgroups of `per` ids each: workgroup g holds 60 isolated bits of block 3 that no other holds, id 3 * B + 65535 twice,
    and ids of block 5 + g % 7"""
    lgrid = min((n + LGRID_IDS - 1) // LGRID_IDS, LGRID_MAX)
    per = (n + lgrid - 1) // lgrid
    s = []
    for g in range(lgrid):
        m = min(per, n - g * per) - 62
        fill = (g * 64 + np.arange(64)) % B
        s += [seg(3, g * 120 + 2 * np.arange(60)), seg(5 + g % 7, fill, m // 64)]
        if m % 64: s.append(seg(5 + g % 7, fill[:m % 64]))
        s.append(seg(3, [B - 1], 2))
    assert spec_len(s) == n
    return s


def _lds(nbl):
    blocks = (0, 4095, 4096, 4097, 8191, 8192, 8193, nbl - 1)
    return [seg(b, [(b * 7) % B, 5, 65535 - j, 5][: 2 + j % 3]) for j, b in enumerate(reversed(blocks))]


def grid_i2():
    c = []
    for base in grid_i1():
        if base.n > 8193: continue
        tag = base.name[3:]
        L = expand(base.spec)
        for order in ("rev", "perm"):
            k = Case("I2/%s/%s" % (order, tag), base.spec, order=order)
            if (np.diff(k.ids().astype(np.int64)) < 0).any(): c.append(k)      # (one id, or equal ids, stay sorted)
        for p in DESCENT_AT:
            s = rotation(L, p)
            if s is not None: c.append(Case("I2/descent_at_%d/%s" % (p, tag), base.spec, order=("rot", p, s), descent=p))
    for n, per in ((LGRID_MAX * LGRID_IDS, 4096), (LGRID_MAX * LGRID_IDS + 1, 4097)):
        c.append(Case("I2/wg512_n_%d" % n, _wg512(n), sorted=False, lgrid=LGRID_MAX, per=per))
    for nbl in LDS_NBL:
        c.append(Case("I2/lds_%d" % nbl, _lds(nbl), nbits=nbl * B - 5, sorted=False, nbl=nbl, lds=nbl <= IDS_LDS_BLOCKS))
    return c


# ---------------------------------------------------------------------------------------------------------------------
# I3: block content, one block per case (block 1), sorted and reversed
# ---------------------------------------------------------------------------------------------------------------------
def block_with_runs(ln, sbit):
    """a block of ln runs whose first run has value sbit: every run 20 bits long but the last 0-run, which takes the rest (so the
    ids stay few)"""
    lens = np.full(ln, 20)
    long_one = ln - 1 if (sbit ^ ((ln - 1) & 1)) == 0 else ln - 2
    lens[long_one] = B - 20 * (ln - 1)
    return block_of_ends(np.cumsum(lens) - 1, sbit)


def _both(c, name, spec, **claims):
    c.append(Case("I3/s/" + name, spec, **claims))
    if np.unique(expand(spec)).size > 1: c.append(Case("I3/u/" + name, spec, order="rev", **claims))


def grid_i3():
    c = []
    for k in IDS_PER_BLOCK:
        o = 5 + 3 * np.arange(k)
        _both(c, "ids_%d_distinct" % k, [seg(1, o)], ids=k)
        s = [seg(1, o[:k // 2], 2)] if k > 1 else []
        if k % 2: s.append(seg(1, o[k // 2:k // 2 + 1]))
        _both(c, "ids_%d_half_duplicates" % k, s, ids=k)
    for ln in RUN_LENS:
        for sbit in (0, 1):
            _both(c, "runs_%d_first_%d" % (ln, sbit), [seg(1, np.flatnonzero(block_with_runs(ln, sbit)))], runs=ln, first=sbit)
    for p in BIT_POS:
        _both(c, "bit_%d" % p, [seg(1, [p])], bits=(p,))
        _both(c, "run_ends_at_%d" % p, [seg(1, np.arange(max(0, p - 40), p + 1))], ends=(p,))
        _both(c, "run_starts_at_%d" % p, [seg(1, np.arange(p, min(B, p + 41)))], starts=(p,))
    _both(c, "bits_at_every_border", [seg(1, BIT_POS)], bits=BIT_POS)
    _both(c, "full", [seg(1, np.arange(B))], ids=B)
    _both(c, "full_plus_duplicates", [seg(1, np.arange(70), 2), seg(1, np.arange(70, B))], ids=B + 70)
    for hole in (0, 30000, B - 1):
        _both(c, "hole_at_%d" % hole, [seg(1, np.delete(np.arange(B), hole))], ids=B - 1)
    return c


# ---------------------------------------------------------------------------------------------------------------------
# I4: touched-block counts around the borders of k_scan_layout
# ---------------------------------------------------------------------------------------------------------------------
def i4_kind(T, t):
    """the kind of touched block t of T under optimize: one FULL block (65,536 ids), three from T = 511, a bit-block (640 ids) every
    5th (T <= 513) or 83rd entry -- both periods coprime to 64, so every lane and step of the scan meets one -- and on the last
    entry; everything else GAP of 1 .. 7 isolated bits"""
    if t == 1 or (T >= 511 and t in (T // 2, T - 2)): return FULL
    if t % (5 if T <= 513 else 83) == 2 or t == T - 1: return BIT
    return GAP


def i4_spec(T):
    s = []
    for t in range(T):
        k, blk = i4_kind(T, t), t + t // 4 + 1                        # an untouched block in front, and after every fourth
        if k == FULL: s.append(seg(blk, np.arange(B)))
        elif k == BIT: s.append(seg(blk, t % 3 + 2 * np.arange(640)))
        else: s.append(seg(blk, t % 50 + 100 * np.arange(1 + t % 7)))
    return s


def grid_i4():
    c = []
    for T in TOUCHED:
        s = i4_spec(T)
        c.append(Case("I4/s/touched_%d" % T, s, touched=T))
        c.append(Case("I4/u/touched_%d" % T, s, order="rev", touched=T))
    return c


# ---------------------------------------------------------------------------------------------------------------------
# I5: windows
# ---------------------------------------------------------------------------------------------------------------------
def _mixed9():
    return [seg(0, [0, 1, 2, 999]), seg(1, 1 + 2 * np.arange(700)), seg(3, np.arange(B)), seg(4, np.arange(100, 30000)),
            seg(5, 2 * np.arange(20000)), seg(7, [B - 1]), seg(8, [0, 17, 65000])]


def i5_windows():
    w = [(f, t) for f in range(10) for t in range(f, 10)]
    return w + [(0, 12), (3, 12), (9, 12), (0, ALL), (4, ALL), (9, ALL)]


def grid_i5():
    s = _mixed9()
    return [Case("I5/s/mixed9", s, nbits=9 * B - 100), Case("I5/u/mixed9", s, nbits=9 * B - 100, order="perm"),
            Case("I5/u/mixed9_sized_by_ids", s, order="rev")]


I5_LDS_WINDOWS = ((0, 16384), (1, 16385), (0, 16385))
I5_PARTITIONS = ((0, 9), (0, 4, 9), (0, 1, 2, 3, 4, 5, 6, 7, 8, 9), (0, 0, 3, 3, 8, 9, 9), (0, 2, 5, 6, 12))


# ---------------------------------------------------------------------------------------------------------------------
# I6: widths and limits
# ---------------------------------------------------------------------------------------------------------------------
def _spec_of(ids):
    return [seg(int(v) >> 16, [int(v) & 0xFFFF]) for v in ids]


W4_HIGH = ((1 << 31) - 1, 1 << 31, (1 << 32) - 65537, (1 << 32) - 1)
W8_HIGH = ((1 << 32) - 1, 1 << 32, (1 << 36) - 1)


def grid_i6():
    c = [Case("I6/w4_high", _spec_of(W4_HIGH)), Case("I6/w4_high_reversed", _spec_of(W4_HIGH), order="rev"),
         Case("I6/w8_high", _spec_of(W8_HIGH), flavour="avx2_64"), Case("I6/w8_high_reversed", _spec_of(W8_HIGH), order="rev", flavour="avx2_64")]
    for tag, mx in (("on", 3 * B - 1), ("off", 3 * B + 6)):
        s = [seg(0, [5, 6]), seg(1, 2 * np.arange(700)), seg(mx >> 16, [mx & 0xFFFF])]
        for what, nbits in (("zero", 0), ("below", mx), ("at", mx + 1), ("above", mx + 2), ("next_block", mx + 1 + B), ("multiple", 6 * B)):
            c.append(Case("I6/nbits_%s_max_%s_a_block_end" % (what, tag), s, nbits=nbits, size=max(nbits, mx + 1)))
    return c


# ---------------------------------------------------------------------------------------------------------------------
_GRIDS = {"I1": grid_i1, "I2": grid_i2, "I3": grid_i3, "I4": grid_i4, "I5": grid_i5, "I6": grid_i6}
N_CASES = {"I1": 29, "I2": 143, "I3": 201, "I4": 24, "I5": 3, "I6": 16}          # cases per grid (checked below)
CASES = {}
for _g, _f in _GRIDS.items():
    _cs = _f()
    assert len({c.name for c in _cs}) == len(_cs) == N_CASES[_g], (_g, len(_cs))
    CASES.update((c.name, c) for c in _cs)
BIG = tuple(sorted(n for n, c in CASES.items() if c.n > PORT_LIMIT))


def grid(name):
    return [c for c in CASES.values() if c.grid == name]


def recorded():
    """the cases that went to the reference (ids_ref.json): the level and threshold cases of I3, I6, every fourth of I1 and I4"""
    r = [c for c in grid("I3") if c.name.startswith("I3/s/runs_") and c.claims["runs"] in LEVEL_LENS] + grid("I6")
    for g in ("I1", "I4"):
        r += [c for c in sorted(grid(g), key=lambda c: c.name)[::4] if c.n <= PORT_LIMIT]
    return r
