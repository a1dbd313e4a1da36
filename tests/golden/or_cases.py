"""Constructed cases for the OR side of the aggregator and for the packed collections (tests/test_or_host.py, tests/test_gpu_or.py):
operands built from explicit run lists so that every border of the row kernel (k_build_tdir / k_agg_or_rows, bmx_kernels7.h),
of the column-tile and direct kernels, of the bags (bmx_kernels6.h), of the member directory (bmx_kernels8.h) and of both
collection builders (bmx_kernels6.h / 10.h) is met on purpose, each with its answer in closed form (the NumPy union).

Geometry.  Vectors have 31 block columns: tile 0 = columns 0 .. 13, tile 1 = columns 14 .. 27, tile 2 = the partial tile 28 .. 30.
  fillers     63 sparse GAP-only operands shared by every list case: filler i holds, in every column c, the three isolated bits
              128 * (10 + 150 k + c) + 2 i (k = 0, 1, 2): its own residue class mod 128, so the filler union is known in closed form
  under test  one operand per case that carries the case in tile 1 (behind the 14 chunks of its tile 0: a non-zero first chunk);
              its tiles 0 and 2 hold fixed decoys (tile 0: a three-word run and a bit per column, i.e. the long flag; tile 2: two
              bits per column), so state left over between rows or tiles shows up.  Uploaded from its block table: it keeps
              exactly the GAP blocks it was built as
  lists       longer than 64 repeat filler handles (unions are idempotent): a large n costs no uploads
A collection case is a list of members whose COLUMNS are the decision points (a column's members are NULL there unless the
column's design gives them a block), built once per role: the AND role takes the complements (0-runs mirror the 1-runs, NULL
<-> FULL), so its answer is the complement of the OR role's.

The model.  tile_record() restates k_build_tdir, bag_layout() the layout of a column of a split collection; the grids are
written against them, and the host test proves through them that a case meets the border it names.  The constants restate
the source (the host test reads the #defines back from the headers).  No GPU, no oracle: pure NumPy."""
import hashlib

import numpy as np

from and_fold_cases import (B, BW, NULL, FULL, BIT, GAP, MAX_GAP_LEN, block_of, block_of_ends, block_with_len, gap_words,  # noqa: F401
                            kind_of, len_sbit, words_of)

NBLOCKS = 31
NBITS = NBLOCKS * B
NW = NBLOCKS * BW

ORR_TILE = 14                          # bmx_kernels7.h: block columns per tile of the row kernel
OR_TILE = 16                           # bmx_kernels2.h: block columns per tile of k_agg_or_gap_tiled
ROW_CHUNKS = 64                        # 16-byte chunks per row: lane L takes chunk L
ROW_WAVES = 16                         # a wave owns every 16th operand ...
ROW_BATCH = 64                         # ... and fetches the records of 64 of them at a time: 1,024 operands per batch
C2_GROUP = 64                          # bmx_kernels10.h: operands per group of the tile build
CM_WAVES = 4                           # bmx_kernels8.h: waves (= items) per workgroup of k_coll_members
QUARTER, ROUND_ENTRIES = 16, 16        # coll_wave_members: four members per step, 16 lanes each; a round = 16 entries per member
WG_SHAPES = (256, 512)                 # k_coll_apply: coll_shape 0, 1 / 2 .. 5
DIRECT_MAX_OPS = 1024                  # bmx_kernels2.h: the direct kernel takes up to 1,024 operands
N_ROWS, N_MEMBERS = 64, 16             # bmx.hip: row / column-tile kernels from 64 operands on, member directory from 16


def bag_round_entries(wg):
    """coll_apply_bag: 4 * WG quads (16 bytes: four 32-bit entries) per round"""
    return 4 * wg * 4


def singles_round(wg):
    """coll_apply_singles: 4 * WG loads of eight 16-bit positions per round"""
    return 4 * wg * 8


def fold_w(wg):
    """coll_fold: words of the difference array per thread; 64 W words per wave"""
    return 2048 // wg


def rows_wanted(gap_words_, gap_blocks):
    """or_rows -1: <= 4.1 chunks of 8 words per GAP block"""
    return gap_blocks > 0 and gap_words_ * 10 <= gap_blocks * 328


def members_wanted(gap_words_, gap_blocks, ops, groups):
    """coll_members -1"""
    return gap_blocks > 0 and gap_words_ <= 48 * gap_blocks and ops >= 32 * groups


TILE1 = range(ORR_TILE, 2 * ORR_TILE)


# ---------------------------------------------------------------------------------------------------------------------
# vectors
# ---------------------------------------------------------------------------------------------------------------------
def _spec(s):
    """a block: None (NULL), "full" (FULL), 65,536 booleans or the GAP words themselves (a GAP block, kept as built)"""
    if s is None or isinstance(s, str):
        assert s is None or s == "full"
        return s
    s = np.asarray(s)
    return gap_words(s) if s.dtype == np.bool_ else s.astype(np.uint16)


def gap_bits(g):
    return block_of_ends(g[1:].astype(np.int64), int(g[0]) & 1)


class Vec:
    """one vector of up to 31 blocks, uploaded from its block table"""
    _next = [0]

    def __init__(self, blocks, note=""):
        self.uid = Vec._next[0]
        Vec._next[0] += 1
        self.note = note
        self.specs = [_spec(s) for s in blocks]
        self.nblocks = len(self.specs)
        assert 0 < self.nblocks <= NBLOCKS
        self.nbits = self.nblocks * B
        self.kinds = tuple(NULL if s is None else FULL if isinstance(s, str) else GAP for s in self.specs)
        for s in self.specs:
            if isinstance(s, np.ndarray): assert (int(s[0]) >> 3) == s.size - 1 and s[-1] == B - 1, note

    def kind(self, c):
        return self.kinds[c] if c < self.nblocks else NULL

    def block(self, c):
        s = self.specs[c] if c < self.nblocks else None
        return np.zeros(B, bool) if s is None else np.ones(B, bool) if isinstance(s, str) else gap_bits(s)

    def words(self):
        """the bits of all 31 columns (columns past the vector's end are empty), from the run lists: edge words by OR, the words
        between them from a difference array (the host test holds this against the plain decode of block())"""
        out = np.zeros(NW, np.uint32)
        S, E = [], []
        for c, s in enumerate(self.specs):
            if s is None: continue
            if isinstance(s, str):
                out[c * BW:(c + 1) * BW] = 0xFFFFFFFF
                continue
            ends = s[1:].astype(np.int64)
            starts = np.concatenate([[0], ends[:-1] + 1])
            one = ((np.arange(ends.size) + (int(s[0]) & 1)) & 1) == 1         # run 1 has the value of the start bit
            S.append(starts[one] + c * B)
            E.append(ends[one] + c * B)
        if S:
            s, e = np.concatenate(S), np.concatenate(E)
            ws, we = s >> 5, e >> 5
            lo, hi = (0xFFFFFFFF << (s & 31)) & 0xFFFFFFFF, 0xFFFFFFFF >> (31 - (e & 31))
            same = ws == we
            np.bitwise_or.at(out, ws[same], (lo & hi)[same].astype(np.uint32))
            np.bitwise_or.at(out, ws[~same], lo[~same].astype(np.uint32))
            np.bitwise_or.at(out, we[~same], hi[~same].astype(np.uint32))
            far = we - ws > 1
            if far.any():
                d = np.zeros(NW + 1, np.int64)
                np.add.at(d, ws[far] + 1, 1)
                np.add.at(d, we[far], -1)
                out[np.cumsum(d[:-1]) > 0] = 0xFFFFFFFF
        return out

    def words_plain(self):
        out = np.zeros(NW, np.uint32)
        for c in range(self.nblocks):
            out[c * BW:(c + 1) * BW] = words_of(self.block(c))
        return out

    def gap_stats(self):
        """(GAP words, GAP blocks): what the host's path selection sums"""
        g = [s for s in self.specs if isinstance(s, np.ndarray)]
        return sum(x.size for x in g), len(g)

    def block_table(self):
        """kinds, offs, bit_slab, gap_slab of the flattened vector"""
        offs, slab, o = [], [], 0
        for s in self.specs:
            offs.append(o if isinstance(s, np.ndarray) else 0)
            if isinstance(s, np.ndarray):
                slab.append(s)
                o += s.size
        return (np.array(self.kinds, np.uint8), np.array(offs, np.uint32), np.zeros(0, np.uint32),
                np.concatenate(slab).astype(np.uint16) if slab else np.zeros(0, np.uint16))

    def complement(self):
        """the same vector in the AND role: every block inverted (NULL <-> FULL, a GAP block with the other start bit)"""
        if not hasattr(self, "_comp"):
            inv = []
            for s in self.specs:
                if isinstance(s, np.ndarray):
                    g = s.copy()
                    g[0] ^= 1
                    inv.append(g)
                else:
                    inv.append("full" if s is None else None)
            self._comp = Vec(inv, note="~" + self.note)
        return self._comp


def gap_of(runs=(), bits=()):
    """the GAP words of a block from its 1-runs [s, e] and single positions (disjoint, never adjacent): block_of + gap_words without
    the 65,536 booleans"""
    r = sorted(list(runs) + [(p, p) for p in bits])
    ends = []
    for s, e in r:
        if s > 0: ends.append(s - 1)
        ends.append(e)
    if not ends or ends[-1] != B - 1: ends.append(B - 1)
    ends = np.array(ends, np.int64)
    assert (np.diff(ends) > 0).all() and ends[0] >= 0
    ln = ends.size
    lvl = 0 if ln <= 124 else 1 if ln <= 252 else 2 if ln <= 508 else 3
    return np.concatenate([[(ln << 3) | (lvl << 1) | int(bool(r) and r[0][0] == 0)], ends]).astype(np.uint16)


def run_counts(bits):
    """(multi-bit, single-bit) 1-runs of a block, straight from its bits"""
    d = np.diff(np.concatenate([[0], bits.astype(np.int8), [0]]))
    ln = np.flatnonzero(d == -1) - np.flatnonzero(d == 1)
    return int((ln > 1).sum()), int((ln == 1).sum())


# ---------------------------------------------------------------------------------------------------------------------
# the model: k_build_tdir, and the layout of a column of a split collection
# ---------------------------------------------------------------------------------------------------------------------
def tile_record(v, t):
    """what k_build_tdir writes for tile t of the vector (and what it counts into bcnt):
      ch        chunks per column of the tile, ceil((len + 1) / 8) for a GAP block, else 0
      nch, M    chunks of the tile, mask of the chunks that start a block (0 for a slow tile)
      gapmask, allgap, long
      slow, why ("chunks": more than 64; "sbit": a block starts with a 1-run; "full": a FULL block)
      first     the tile's first chunk in the slab (GAP blocks lie back to back on 16-byte boundaries, in block order)
      multi, single   per column the runs bcnt holds (None for the GAP blocks of a slow tile: 0xFFFFFFFF there)
      multi_pairs     (chunk of the tile, pair of the chunk) of every multi-bit run"""
    ch, why, stream = [0] * ORR_TILE, set(), []
    nch = M = gapmask = 0
    for k in range(ORR_TILE):
        c = t * ORR_TILE + k
        kind = v.kind(c)
        if kind == GAP:
            g = v.specs[c]
            ln = int(g[0]) >> 3
            n = (ln + 1 + 7) >> 3
            if int(g[0]) & 1: why.add("sbit")
            if nch < 64: M |= 1 << nch
            gapmask |= 1 << k
            ch[k] = n
            nch += n
            pad = np.full(n * 8, 0xFFFF, np.int64)             # the padding every writer of a slab sees to
            pad[:ln + 1] = g
            stream.append(pad)
        elif kind != NULL:
            why.add("full")
    if nch > ROW_CHUNKS: why.add("chunks")
    slow = bool(why)
    first = 0
    for c in range(t * ORR_TILE):
        if v.kind(c) == GAP: first += (v.specs[c].size + 7) >> 3
    rec = dict(ch=ch, nch=nch, M=0 if slow else M, gapmask=gapmask, allgap=gapmask == (1 << ORR_TILE) - 1, slow=slow,
               why=tuple(sorted(why)), long=False, first=first, multi=[0] * ORR_TILE, single=[0] * ORR_TILE, multi_pairs=[])
    if slow:
        for k in range(ORR_TILE):
            if (gapmask >> k) & 1: rec["multi"][k] = rec["single"][k] = None
    elif nch:
        # the word pairs (2 i + 1, 2 i + 2) of every chunk, the last one reaching into the next chunk (behind the tile: 0xFFFF)
        s = np.concatenate(stream + [[0xFFFF]])
        p, e = s[1::2][:nch * 4], s[2::2][:nch * 4]
        run = p != 0xFFFF
        one = run & (e - p == 1)
        owner = np.repeat(np.arange(ORR_TILE), ch)[np.arange(nch * 4) // 4]
        for k in range(ORR_TILE):
            rec["multi"][k] = int((run & ~one & (owner == k)).sum())
            rec["single"][k] = int((one & (owner == k)).sum())
        rec["multi_pairs"] = [(int(i) // 4, int(i) % 4) for i in np.flatnonzero(run & ~one)]
        rec["long"] = bool(rec["multi_pairs"])
    return rec


def nth_set_bit16(m, r):
    """position of the r-th (0-based) set bit of a 16-bit mask"""
    return [k for k in range(16) if (m >> k) & 1][r]


def bag_layout(nm, ns):
    """a column of a split collection: nm multi-bit entries (32 bits each) padded to 4, then ns 16-bit positions padded to 8"""
    return dict(nm=nm, ns=ns, singles_at=(nm + 3) & ~3, words=((nm + 3) & ~3) + (((ns + 7) & ~7) >> 1), pad_m=-nm % 4, pad_s=-ns % 8)


def column_counts(members, c):
    """(multi-bit, single-bit) entries of every member's piece of column c"""
    return [run_counts(m.block(c)) if m.kind(c) == GAP else (0, 0) for m in members]


# ---------------------------------------------------------------------------------------------------------------------
# fillers, decoys, the operand under test
# ---------------------------------------------------------------------------------------------------------------------
N_FILLERS = 63
_FILLERS, _WORDS = [], {}


def filler_bits(i, c):
    return [128 * (10 + 150 * k + c) + 2 * i for k in range(3)]


def fillers():
    if not _FILLERS:
        for i in range(N_FILLERS):
            _FILLERS.append(Vec([gap_of((), filler_bits(i, c)) for c in range(NBLOCKS)], note="filler%d" % i))
            _WORDS[_FILLERS[-1].uid] = _FILLERS[-1].words()
    return _FILLERS


def filler_union(which=range(N_FILLERS)):
    """the closed form of the union of the given fillers"""
    pos = [c * B + p for c in range(NBLOCKS) for i in which for p in filler_bits(i, c)]
    bits = np.zeros(NBITS, bool)
    bits[pos] = True
    return words_of(bits)


_DECOY0 = [gap_words(block_of([(5000 + c, 5070 + c)], [40000 + c])) for c in range(ORR_TILE)]
_DECOY2 = [gap_words(block_of((), [777 + k, 60001])) for k in range(NBLOCKS - 2 * ORR_TILE)]
_PLAIN1 = [gap_words(block_of((), [30000 + c])) for c in range(ORR_TILE)]          # one chunk, one single-bit run


def rich(c):
    """a tile-1 block with a two-word run and two bits: one chunk"""
    return block_of([(1000 + c, 1040 + c)], [20000 + c, 20002 + c])


def xvec(tile1=None, nblocks=NBLOCKS, note="", default=_PLAIN1):
    """the operand under test: decoys in tiles 0 and 2, tile 1 from {column of the tile: block} over the default blocks"""
    t1 = list(default)
    for k, s in (tile1 or {}).items():
        t1[k] = s
    return Vec((_DECOY0 + t1 + _DECOY2)[:nblocks], note=note)


def union_words(ops):
    out = np.zeros(NW, np.uint32)
    for o in {o.uid: o for o in ops}.values():
        out |= _WORDS[o.uid] if o.uid in _WORDS else o.words()
    return out


def kinds_of_union(words, ops, opt):
    """block kinds of a combine_or result.  opt_none: bit-blocks, FULL where a FULL operand saturates the column, NULL where
    nothing is set; opt_compress: one run -> NULL / FULL, fewer than 1,276 runs -> GAP"""
    full = {c for o in ops for c in range(o.nblocks) if o.kinds[c] == FULL}
    out = []
    for c in range(NBLOCKS):
        w = words[c * BW:(c + 1) * BW]
        if c in full: out.append(FULL)
        elif not w.any(): out.append(NULL)
        elif not opt: out.append(BIT)
        else: out.append(kind_of(np.unpackbits(w.view(np.uint8), bitorder="little").astype(bool)))
    return out


def sha(words):
    return hashlib.sha256(np.ascontiguousarray(words, np.uint32).tobytes()).hexdigest()


class Case:
    """one list case: the operand list (fillers included, in list order), the operand under test and what the model must say
    about its tile 1 (claims), the values the case stands for in its grid (params)"""

    def __init__(self, grid, name, ops, x=None, claims=None, **params):
        self.grid, self.name, self.ops, self.x, self.claims, self.params = grid, name, list(ops), x, claims or {}, params

    def __repr__(self):
        return "%s/%s n=%d %s" % (self.grid, self.name, len(self.ops), " ".join("%s=%s" % kv for kv in self.params.items()))

    def expect(self, ops=None):
        """words, count, kinds under opt_none, kinds under opt_compress of the union of the list (or of a part of it)"""
        ops = self.ops if ops is None else ops
        w = union_words(ops)
        return w, int(np.unpackbits(w.view(np.uint8)).sum()), kinds_of_union(w, ops, False), kinds_of_union(w, ops, True)


def o1_list(x, *more):
    """64 operands (+ more): the operand under test at index 5, so that the first 63 operands of the list hold it too"""
    f = fillers()
    return f[:5] + [x] + list(more) + f[5:]


# ---------------------------------------------------------------------------------------------------------------------
# O1: row geometry
# ---------------------------------------------------------------------------------------------------------------------
def o1_lens():
    """len at every residue mod 8 at one, two and three chunks, and next to the longest GAP block an import keeps"""
    return list(range(1, 25)) + list(range(MAX_GAP_LEN - 7, MAX_GAP_LEN + 1))


O1_COLS = (0, 7, 13)
O1_MASKS = dict([("col0", 1), ("col13", 1 << 13), ("even", 0x1555), ("odd", 0x2AAA), ("none", 0)] +
                [("allbut%d" % p, 0x3FFF & ~(1 << p)) for p in range(ORR_TILE)])
O1_NBLOCKS = (14, 15, 21, 27, 28)
SHAPES = {"bit1": ((), (1,)), "bit31": ((), (31,)), "bit32": ((), (32,)), "bit65534": ((), (65534,)), "bit65535": ((), (65535,)),
          "two.in": (((40, 41),), ()), "two.across": (((31, 32),), ()), "twowords": (((32, 95),), ()),
          "threewords": (((32, 127),), ()), "allbut0": (((1, 65535),), ())}
# (len, start bit) of the blocks whose last run ends at 65535 as a 1-run / a 0-run with (len + 1) % 8 == 0 / == 1.  With start
# bit 0 run k is a 1-run for even k: a last 1-run needs an even len, so (len + 1) % 8 == 0 takes the start bit 1 (a slow tile)
ENDS = {"end1.r0": (7, 1), "end1.r1": (8, 0), "end0.r0": (7, 0), "end0.r1": (8, 1)}


def singles_block(pos, multi=()):
    """single bits at pos; the (1-based) run numbers in multi are two bits wide"""
    return block_of([(p, p + 1) for j, p in enumerate(pos, 1) if j in multi], [p for j, p in enumerate(pos, 1) if j not in multi])


def grid_o1():
    cases = []

    def one(name, tile1, claims, more=(), nblocks=NBLOCKS, **params):
        x = xvec(tile1, nblocks, note="o1." + name)
        cases.append(Case("O1", name, o1_list(x, *more), x, claims, **params))

    def why_of(sb, nch):
        return tuple(sorted((["sbit"] if sb else []) + (["chunks"] if nch > ROW_CHUNKS else [])))

    # block length x start bit x column of the tile (every column at the lens whose last chunk is full or holds one word)
    for ln in o1_lens():
        for sb in (0, 1):
            if (ln, sb) == (1, 1): continue                 # (all ones as one GAP run: an import makes a FULL block of it)
            for col in (O1_COLS if (ln + 1) % 8 in (0, 1) else (O1_COLS[(ln + sb) % 3],)):
                nch = ORR_TILE - 1 + ((ln + 8) >> 3)
                why = why_of(sb, nch)
                one("len%d.%d.c%d" % (ln, sb, col), {col: block_with_len(ln, sb)}, dict(nch=nch, slow=bool(why), why=why),
                    len=ln, sbit=sb, col=col)
    # tile totals of 63, 64, 65 chunks: 13 blocks of 4 chunks + one of 11 / 12 / 13, the long block first and last
    four = {c: block_with_len(24 + c % 8, 0) for c in range(ORR_TILE)}
    for tot, big in ((63, 87), (64, 95), (65, 103)):
        for pos in (0, 13):
            t = dict(four)
            t[pos] = block_with_len(big, 0)
            why = why_of(0, tot)
            one("total%d.long%d" % (tot, pos), t, dict(nch=tot, slow=bool(why), why=why, long=None if why else True), total=tot, longpos=pos)
    # 64 chunks, chunk 63 = the last chunk of the last block: len 30 -- its last pair that can hold a run (words 5, 6) is the
    # 1-run ending at 65535; len 31 -- the pair is a run and word 7 is the block's last word (lane 63's successor: "no run")
    for ln in (30, 31):
        t = dict(four)
        t[0], t[13] = block_with_len(95, 0), block_with_len(ln, 0)
        one("total64.last%d" % ln, t, dict(nch=64, slow=False, why=(), lane63_pair2=True), total=64, lastlen=ln)
    # tiles that are not all-GAP
    for name, mask in O1_MASKS.items():
        t = {k: (rich(k) if (mask >> k) & 1 else None) for k in range(ORR_TILE)}
        one("mask." + name, t, dict(gapmask=mask, allgap=False, slow=False, nch=bin(mask).count("1")), mask=name)
    for col in O1_COLS:
        t = {k: rich(k) for k in range(ORR_TILE)}
        t[col] = "full"
        one("full.c%d" % col, t, dict(slow=True, why=("full",), gapmask=0x3FFF & ~(1 << col)), full=col, fullwith=0)
        other = xvec({col: rich(col)}, note="o1.full.other%d" % col)
        one("full+runs.c%d" % col, t, dict(slow=True, why=("full",)), more=(other,), full=col, fullwith=1)
    # operands shorter than the list
    for nb in O1_NBLOCKS:
        t = {k: rich(k) for k in range(ORR_TILE)}
        one("nblocks%d" % nb, t, dict(gapmask=(1 << max(0, min(ORR_TILE, nb - ORR_TILE))) - 1, slow=False), nblocks=nb, nblocks_=nb)
    # the long flag: every run of the tile one bit, against exactly one multi-bit run -- in pair 0 of chunk 0, in pair 3 of chunk 0
    # (words 7 and 8: the pair reaches into the block's next chunk), in the last chunk of the tile
    pos = [1000 * j + 17 for j in range(1, 7)]                  # 6 runs: len 13, two chunks
    one("long.clear", {0: singles_block(pos), 13: singles_block(pos)}, dict(long=False, nch=16, slow=False), long="clear")
    for tag, col, run, pair in (("pair0", 0, 1, (0, 0)), ("pair3", 0, 4, (0, 3)), ("lastchunk", 13, 5, (15, 0))):
        one("long." + tag, {0: singles_block(pos, (run,) if col == 0 else ()), 13: singles_block(pos, (run,) if col == 13 else ())},
            dict(long=True, nch=16, slow=False, multi_pairs=[pair]), long=tag)
    # run shapes in the block under test
    for name, (runs, bits) in SHAPES.items():
        for col in (7, 13):
            one("shape.%s.c%d" % (name, col), {col: block_of(runs, bits)}, dict(slow=False, nch=ORR_TILE), shape=name, col=col)
    for name, (ln, sb) in ENDS.items():
        for col in (7, 13):
            nch = ORR_TILE - 1 + ((ln + 8) >> 3)
            one("shape.%s.c%d" % (name, col), {col: block_with_len(ln, sb)}, dict(slow=bool(sb), nch=nch), shape=name, col=col)
    # a run that shares a word with a filler's bits: a bit between two fillers' bits, and a run over three of them
    c = ORR_TILE + 7
    p = filler_bits(0, c)[0]
    one("shape.shared.c7", {7: block_of([(p + 5, p + 9)], [p + 1])}, dict(slow=False, long=True), shape="shared", col=7)
    return cases


# ---------------------------------------------------------------------------------------------------------------------
# O2: who owns which operand
# ---------------------------------------------------------------------------------------------------------------------
O2_N = (64, 65, 79, 80, 81, 127, 128, 1023, 1024, 1025, 1040, 2049)
O2_IDX = (0, 1, 15, 16, 17, 1008, 1023, 1024)


def fill(n, placed):
    """a list of n operands: the placed ones at their indices, fillers in turn everywhere else"""
    f, out, j = fillers(), [], 0
    for i in range(n):
        if i in placed:
            out.append(placed[i])
        else:
            out.append(f[j % N_FILLERS])
            j += 1
    return out


def grid_o2():
    t = {k: rich(k) for k in range(ORR_TILE)}
    t[3], t[9] = None, singles_block([1000 * j + 17 for j in range(1, 7)], (4,))
    xa = xvec(t, note="o2.x")
    xb = xvec({k: block_of([(3000 + k, 3100 + k)], [50000 + k]) for k in range(ORR_TILE)}, note="o2.x2")
    z = Vec([None] * NBLOCKS, note="o2.null")                   # no GAP block: no tile directory, dropped from the operand table
    cases = []
    for n in O2_N:
        for idx in sorted({i for i in O2_IDX if i < n} | {n - 1}):
            cases.append(Case("O2", "n%d.i%d" % (n, idx), fill(n, {idx: xa}), xa, {}, n=n, idx=idx, nulls=0, second=None))
    for n, idx in ((64, 20), (81, 16), (1025, 1023)):
        for k in (1, 2, 3):
            for where, at in (("before", [idx - 1 - j for j in range(k)]), ("between", [idx - 1, idx + 1, idx - 2][:k]),
                              ("after", [idx + 1 + j for j in range(k)])):
                placed = {i: z for i in at if 0 <= i < n}
                placed[idx] = xa
                cases.append(Case("O2", "n%d.i%d.null%d.%s" % (n, idx, k, where), fill(n, placed), xa, {}, n=n, idx=idx, nulls=len(placed) - 1,
                                  where=where, second=None))
    for n in (1040, 2049):
        for idx in (0, 15):
            for tag, d in (("batch", ROW_WAVES), ("next", ROW_WAVES * ROW_BATCH)):
                if idx + d < n:
                    cases.append(Case("O2", "n%d.i%d.second.%s" % (n, idx, tag), fill(n, {idx: xa, idx + d: xb}), xa, {}, n=n, idx=idx,
                                      nulls=0, second=tag))
    return cases


# ---------------------------------------------------------------------------------------------------------------------
# O3 .. O5: collections.  columns[c] = {member: block}; everything else is NULL
# ---------------------------------------------------------------------------------------------------------------------
class Coll:
    """a member list built from column designs.  notes[c]: what column c is there for"""

    def __init__(self, name, n, columns, notes, nblocks=NBLOCKS):
        self.name, self.n, self.notes = name, n, notes
        per = [[None] * nblocks for _ in range(n)]
        for c, d in columns.items():
            for i, s in d.items():
                assert per[i][c] is None, (name, c, i)
                per[i][c] = s
        self.members = [Vec(b, note="%s.m%d" % (name, i)) for i, b in enumerate(per)]
        self._w = self._wa = None

    def words(self, role="or"):
        """(n, NW) words of the members in the role (cached; the AND role is the complement)"""
        if self._w is None:
            self._w = np.stack([m.words() for m in self.members])
        if role == "or":
            return self._w
        if self._wa is None:
            self._wa = ~self._w
            for i, m in enumerate(self.members):
                self._wa[i, m.nblocks * BW:] = 0
        return self._wa

    def vecs(self, role="or"):
        return self.members if role == "or" else [m.complement() for m in self.members]

    def union(self, idx=None):
        w = self.words()
        return np.bitwise_or.reduce(w if idx is None else w[sorted(set(idx))], axis=0)

    def counts(self, c):
        return column_counts(self.members, c)

    def totals(self, c):
        k = self.counts(c)
        return sum(m for m, s in k), sum(s for m, s in k)


O3_NM = tuple(c % 10 for c in range(NBLOCKS))
O3_NS = tuple((7 * c) % 18 for c in range(NBLOCKS))


def coll_bags(n=66):
    """O3: per column nm multi-bit and ns single-bit entries (0 .. 9 x 0 .. 17: every residue mod 4 and mod 8, columns with only
    singles, only multis, neither -- column 0 -- and, in column 30, a FULL member), two entries per member"""
    cols, notes = {}, {}
    for c in range(NBLOCKS):
        nm, ns = O3_NM[c], O3_NS[c]
        ent = [("m", k) for k in range(nm)] + [("s", j) for j in range(ns)]
        per = {}
        for e, (what, k) in enumerate(ent):
            i = (3 * c + e // 2) % n
            runs, bits = per.setdefault(i, ([], []))
            if what == "m": runs.append((2048 * (k + 1) + 70 * c + 3, 2048 * (k + 1) + 70 * c + 4 + 7 * k))
            else: bits.append(30000 + 1000 * k + c)
        cols[c] = {i: block_of(r, b) for i, (r, b) in per.items()}
        notes[c] = "nm=%d ns=%d" % (nm, ns)
    cols[30][50] = "full"
    notes[30] += " + a FULL member"
    used = {i for d in cols.values() for i in d}
    for i in range(n):                                          # (a larger collection: no member without a block -- a bit in column 1)
        if i not in used: cols[1][i] = block_of((), [60000 + i])
    return Coll("bags", n, cols, notes)


FOLD_BOUNDS = (40, 44, 256, 512)       # k W for W = 8 and 4 (40), for W = 4 alone (44); the wave boundaries 64 W = 256 and 512
FOLD_COLS = dict(shapes=0, b40=1, b44=2, b256=3, b512=4, w2047=5, stack2=6, stack3=7, stack64=8, abut=9, multis1=10, multis2=11,
                 singles1=12, full=20, sbit=21, edges=22)
HEAVY_RUNS, HEAVY_BITS = 130, 260


def fold_runs(b):
    """the six runs around the word boundary b: interiors whose first / last covered word is b - 1, b, b + 1"""
    out = []
    for d in (-1, 0, 1):
        f = b + d
        out.append(("first", d, (32 * (f - 1) + 7, 32 * (f + 2) + 9)))      # interior words f, f + 1
        out.append(("last", d, (32 * (f - 2) + 5, 32 * (f + 1) + 3)))       # interior words f - 1, f
    return out


def interior(run):
    """the interior words of a run (those coll_fold covers): (first, last) or None"""
    ws, we = run[0] >> 5, run[1] >> 5
    return (ws + 1, we - 1) if we - ws > 1 else None


def coll_fold_(n=130):
    """O3: run shapes as entries, coll_fold's thread and wave boundaries, stacked and abutting interiors, columns with more
    entries than one / two rounds of coll_apply_bag and one round of coll_apply_singles hold; members with slow tiles (more than
    64 chunks, a FULL block, start bit 1) among members with fast ones"""
    F, cols, notes = FOLD_COLS, {}, {}
    cols[F["shapes"]] = {i: block_of(*SHAPES[k]) for i, k in enumerate(SHAPES)}
    for b in FOLD_BOUNDS:
        cols[F["b%d" % b]] = {10 + j: block_of([run]) for j, (_, _, run) in enumerate(fold_runs(b))}
    cols[F["w2047"]] = {16: block_of([(32 * 2040 + 5, B - 1)]), 17: block_of([(32 * 2046 + 1, B - 1)])}
    for tag, m in (("stack2", 2), ("stack3", 3), ("stack64", 64)):
        cols[F[tag]] = {(18 if m < 64 else 0) + i: block_of([(32 * 100 + i % 32, 32 * 110 + (7 * i) % 32)]) for i in range(m)}
    cols[F["abut"]] = {23: block_of([(32 * 200 + 5, 32 * 203 + 4)]), 24: block_of([(32 * 202 + 9, 32 * 206 + 1)])}
    heavy = lambda i: block_of([(500 * k + 4 * (i % 100), 500 * k + 4 * (i % 100) + 1) for k in range(HEAVY_RUNS)])
    cols[F["multis1"]] = {i: heavy(i) for i in range(64)}
    cols[F["multis2"]] = {i: heavy(i + 7) for i in range(128)}
    cols[F["singles1"]] = {i: block_of((), [250 * k + 2 * (i % 100) for k in range(HEAVY_BITS)]) for i in range(64)}
    cols[F["full"]] = {30: "full", 31: block_of([(100, 300)], [500])}
    cols[F["sbit"]] = {32: block_of([(0, 100)], [7000]), 35: block_of((), [7001])}
    cols[F["edges"]] = {33: block_of([(0, 777)]), 34: block_of([(50000, B - 1)])}
    for i in range(n):                                          # a bit of its own for every member
        cols.setdefault(13 + i % 7, {})[i] = block_of((), [60000 + i])
    for k, c in F.items(): notes[c] = k
    return Coll("fold", n, cols, notes)


O4_COUNTS = (0, 1, 15, 16, 17, 32, 33)
O4_M = (1, 3, 4, 5, 15, 16, 17, 63, 64, 65, 128, 129)
O4_POS = (0, 3, 4, 15, 16, 63, 64)
O4_SIZES = (31, 32, 33, 63, 64, 65)
O4_GROUPS = (1, 3, 4, 5)
O4_T0 = 100                             # members 100 .. 106 are the members under test


def o4_piece(k, c):
    """(multi-bit, single-bit) entries of member O4_T0 + k in column c: every pair of O4_COUNTS occurs"""
    return O4_COUNTS[(k + c) % 7], O4_COUNTS[(k + 3 + 2 * c) % 7]


def coll_dir(n=200, nblocks=NBLOCKS, name="dir"):
    """O4: every member three bits per column (256 (5 + 75 k + c) + i); the members under test hold the pieces of o4_piece"""
    cols = {}
    for c in range(nblocks):
        d = {}
        for i in range(n):
            k = i - O4_T0
            if 0 <= k < 7:
                em, es = o4_piece(k, c)
                if em + es:
                    d[i] = gap_of([(40000 + 600 * j + 8 * k, 40000 + 600 * j + 8 * k + 3) for j in range(em)],
                                  [40300 + 600 * j + 8 * k for j in range(es)])
            else:
                d[i] = gap_of((), [256 * (5 + 75 * j + c) + i for j in range(3)])
        cols[c] = d
    return Coll(name, n, cols, {}, nblocks)


def o4_lists():
    """(m, position of the member under test, which one, order, member indices): the member at its position among others"""
    others = [i for i in range(200) if not 0 <= i - O4_T0 < 7]
    out, k = [], 0
    for m in O4_M:
        for p in O4_POS:
            if p >= m: continue
            rest = others[k:k + m - 1]
            lst = rest[:p] + [O4_T0 + k % 7] + rest[p:]
            out.append((m, p, k % 7, "asis", lst))
            k += 1
    for m, p, t, _, lst in list(out):
        if m in (5, 17, 65, 129) and p == 0:
            out.append((m, m - 1, t, "reverse", lst[::-1]))
            out.append((m + 3, p, t, "repeats", lst + lst[:3]))
    return out


def o4_pipelines():
    """groups (AND list from the AND-role collection, SUB list from the OR-role one) of the pipelines of 1, 3, 4 and 5 groups"""
    ls = [l for l in o4_lists() if l[0] >= 3]
    out, k = [], 0
    for g in O4_GROUPS:
        groups = []
        for j in range(g):
            a, s = ls[(k + j) % len(ls)][4], ls[(k + j + 11) % len(ls)][4]
            groups.append((a[:max(1, len(a) // 8)], s))
        out.append(groups)
        k += g
    return out


_COLLS = {}


def coll(name):
    if name not in _COLLS:
        if name == "bags": c = coll_bags()
        elif name == "fold": c = coll_fold_()
        elif name == "dir": c = coll_dir()
        elif name == "short": c = coll_dir(40, 20, "short")                       # fewer columns than the pipelines over it
        elif name.startswith("dir"): c = coll_dir(int(name[3:]), name=name)       # O4_SIZES, and both sides of C2_GROUP
        elif name.startswith("bags"): c = coll_bags(int(name[4:]))
        else: raise KeyError(name)
        _COLLS[name] = c
    return _COLLS[name]


O5_SIZES = (64, 65, 128, 129)
COLLS_FULL = ("bags", "fold") + tuple("bags%d" % n for n in O5_SIZES)              # full-list cases (O3, O5)
COLLS_DIR = ("dir",) + tuple("dir%d" % n for n in O4_SIZES)                       # member-directory cases (O4)


# ---------------------------------------------------------------------------------------------------------------------
# O6: the pattern a producer that can express arbitrary content is asked for
# ---------------------------------------------------------------------------------------------------------------------
def o6_pattern(j=0):
    """31 blocks; tile 1 holds blocks of every (len + 1) % 8 (one and two chunks), a NULL column and a FULL column; j moves the
    bits so that several producers give different operands.  -> (blocks, bits of the whole vector)"""
    blocks = []
    for c in range(NBLOCKS):
        k = c - ORR_TILE
        if 0 <= k < 12:
            ln = 6 + k                                          # len 6 .. 17: every (len + 1) % 8, one to three chunks
            pos = [3000 + 900 * i + 3 * j + c for i in range(ln // 2 - (ln % 2 == 0))]
            b = block_of([(pos[0], pos[0] + 40)] if k % 3 == 1 else (), pos)
            if ln % 2 == 0: b[B - 1] = True                     # even len: the last run is a 1-run up to 65535
            assert len_sbit(b) == (ln, 0)
        elif k == 12: b = np.zeros(B, bool)
        elif k == 13: b = np.ones(B, bool)
        else: b = block_of([(5000 + c + j, 5070 + c + j)], [40000 + c + 2 * j, 777 + c])
        blocks.append(b)
    return blocks, np.concatenate(blocks)


def o6_residues():
    return sorted({(len_sbit(b)[0] + 1) % 8 for b in o6_pattern()[0][ORR_TILE:ORR_TILE + 12]})


def ranges_of(bits):
    d = np.diff(np.concatenate([[0], bits.astype(np.int8), [0]]))
    return np.stack([np.flatnonzero(d == 1), np.flatnonzero(d == -1) - 1], axis=1).astype(np.uint64)


# ---------------------------------------------------------------------------------------------------------------------
# grids, chunks, caches
# ---------------------------------------------------------------------------------------------------------------------
_GRIDS = {"O1": grid_o1, "O2": grid_o2}
_CACHE = {}
N_CASES = {"O1": 166, "O2": 117}            # cases per grid (checked when a grid is built)
CHUNK = {"O1": 8, "O2": 8}            # cases per parametrised test


def grid(name):
    if name not in _CACHE:
        _CACHE[name] = _GRIDS[name]()
        assert len(_CACHE[name]) == N_CASES[name], (name, len(_CACHE[name]))
    return _CACHE[name]


def chunks():
    return [(g, k) for g in _GRIDS for k in range((N_CASES[g] + CHUNK[g] - 1) // CHUNK[g])]


def chunk(name, k):
    return grid(name)[k * CHUNK[name]:(k + 1) * CHUNK[name]]


def port_vec(orc, v, cache):
    """the vector inside an oracle: the port takes the block table as built, the reference imports the bits (a GAP block of one
    run becomes NULL / FULL there: the same bits)"""
    key = (orc.is_ref, v.uid)
    if key not in cache:
        if orc.is_ref:
            cache[key] = orc.import_words(v.words()[:v.nblocks * BW], True, v.nbits)
        else:
            cache[key] = orc.from_table(v.nbits, *v.block_table())
    return cache[key]


def device_vec(bm, ctx, v, cache):
    """uploaded from its block table: the device vector holds exactly the blocks the case was built with"""
    key = (id(ctx), v.uid)
    if key not in cache:
        cache[key] = bm.bvector.from_block_table(ctx, v.nbits, *v.block_table())
    return cache[key]


# ---------------------------------------------------------------------------------------------------------------------
# the fixture (tests/golden/or_ref.json): a fixed subset, as the reference computes it
# ---------------------------------------------------------------------------------------------------------------------
RECORD = {"O1": 4, "O2": 6}             # every RECORD[g]-th case of a grid is recorded


def recorded():
    """(key, operands) of the recorded results: list cases, and the full list of every O3 / O5 collection"""
    out = [("%s/%s" % (g, c.name), c.ops) for g in _GRIDS for c in grid(g)[1::RECORD[g]]]
    return out + [("coll/%s" % n, coll(n).members) for n in COLLS_FULL]


def kinds_str(kinds):
    return "".join("%d" % k for k in kinds)


def oracle_fixture(orc, cache=None):
    cache = {} if cache is None else cache
    out = {}
    for key, ops in recorded():
        pv = [port_vec(orc, o, cache) for o in ops]
        e = {}
        for opt in (False, True):
            r = orc.agg_or(pv, opt)
            e["compress" if opt else "none"] = {"kinds": kinds_str((r.flatten()[0].tolist() + [0] * NBLOCKS)[:NBLOCKS]), "count": r.count(),
                                                "sha": sha(r.to_words(NW))}
        out[key] = e
    return {"cases": out}
