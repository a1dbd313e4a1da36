"""Constructed cases for build_rs_index / rank / select: every case is an explicit sorted list of one-positions with its size, the
tuning keys of the build and the query lists; the answers are closed forms over that list (rank_expect / select_expect), and a small
integer model restates what the build decides (sample shift, select-line width, directory shift and entries, summary shape, P8,
group spread, fb, "summary dropped", the first guess of k_select_top), so that rs_index.info() is predicted exactly.  Pure NumPy:
no oracle, no device.  tests/test_rs_host.py checks the model's claims and the reference fixture (rs_ref.json, written by
make_rs_golden.py); tests/test_gpu_rs.py runs the kernels.

Grid A  placements: every block class against two predecessors, exhaustive rank and select, dead queries, short batches.
Grid B  select lines: the 16 / 32-bit switch at a span of 65,535 | 65,536 bits, counts around K, the staging passes of the
        writer, the policy expression, the 2^32 unit border.
Grid C  select directory and LDS summary: entry borders, skewed entries (secant steps, then bisection), a batch whose first
        guesses miss (the parked-query queue), the summary's precision fb at each threshold, the summary shift at 65,536 entries.
Grid D  block search of the table kernels: carriers among NULL blocks around the sample-group borders, from 1 to 131,073 blocks."""
from __future__ import annotations

import hashlib

import numpy as np

B = 65536
RL_LINES, RL_BITS = 69, 960
STOP_ENTRIES, STOP_GROUP, STOP_BYTES = 65536, 64, 135168
SL_BYTES = 128
U64 = np.uint64
REF_LIMIT = (1 << 32) - 1                       # a 32-bit reference build addresses bits 0 .. 2^32 - 2

KEYS0 = {"rs_lines": 0, "rs_select_sel": 0, "rs_sdir_shift": 6}


class Case:
    def __init__(self, name, nbits, ones, keys, rank_q=None, select_r=None, batches=(), claims=None):
        self.name, self.nbits = name, int(nbits)
        self.ones = np.ascontiguousarray(ones, U64)
        assert self.ones.size == 0 or ((np.diff(self.ones.astype(np.int64)) > 0).all() and int(self.ones[-1]) < self.nbits), name
        self.keys = dict(KEYS0); self.keys.update(keys)
        self.nblocks = (self.nbits + B - 1) // B
        self.count = int(self.ones.size)
        self.rank_q = dead_positions(self) if rank_q is None else np.ascontiguousarray(rank_q, U64)
        self.select_r = np.concatenate([np.arange(1, self.count + 1, dtype=U64), dead_ranks(self)]) if select_r is None else np.ascontiguousarray(select_r, U64)
        self.batches = tuple(batches)           # batch sizes: prefixes of the (shuffled) select list, and of the rank list
        self.claims = claims or {}              # what the case is built to show; the host test holds the model to it

    def fits_reference(self):
        return self.nbits <= REF_LIMIT + 1 and (self.count == 0 or int(self.ones[-1]) < REF_LIMIT)

    def ref_rank_q(self):
        return self.rank_q[self.rank_q < U64(REF_LIMIT)]

    def ref_select_r(self):
        return self.select_r[self.select_r < U64(REF_LIMIT)]

    def __repr__(self):
        return "rs case %s (%d blocks, %d ones)" % (self.name, self.nblocks, self.count)


# ---- closed forms ----
def rank_expect(c, q):
    q = np.asarray(q, U64)
    r = np.searchsorted(c.ones, q, "right").astype(U64)
    return np.where((q >> U64(16)) >= U64(c.nblocks), U64(c.count), r)


def select_expect(c, r):
    """-> (found, pos); not found answers position 0"""
    r = np.asarray(r, U64)
    ok = (r >= U64(1)) & (r <= U64(c.count))
    at = np.where(ok, r - U64(1), U64(0)).astype(np.int64)
    pos = np.where(ok, c.ones[at] if c.count else U64(0), U64(0)).astype(U64)
    return ok, pos


def bit_expect(c, n):
    n = np.asarray(n, U64)
    i = np.searchsorted(c.ones, n, "left")
    return (i < c.count) & (c.ones[np.minimum(i, max(c.count - 1, 0))] == n) if c.count else np.zeros(n.shape, bool)


def count_range_expect(c, l, r):
    l, r = np.asarray(l, U64), np.asarray(r, U64)
    lo, hi = np.minimum(l, r), np.maximum(l, r)
    return (np.searchsorted(c.ones, hi, "right") - np.searchsorted(c.ones, lo, "left")).astype(U64)


def find_rank_expect(c, rank, frm):
    rank, frm = np.asarray(rank, U64), np.asarray(frm, U64)
    before = np.searchsorted(c.ones, frm, "left").astype(U64)
    return select_expect(c, np.where(rank > 0, rank + before, U64(0)))


def dead_positions(c):
    return np.array([c.nbits, c.nbits + 70000, 1 << 36, (1 << 64) - 1], U64)


def dead_ranks(c):
    return np.array([0, c.count + 1, 1 << 40], U64)


def around(c, pos):
    """every position, the one before it and the one after it (inside the vector)"""
    p = np.asarray(pos, np.int64)
    q = np.unique(np.concatenate([p, p - 1, p + 1]))
    return q[(q >= 0) & (q < c.nbits)].astype(U64)


def sha(a, dtype=U64):
    return hashlib.sha256(np.ascontiguousarray(a, dtype).tobytes()).hexdigest()


def runs_of(ones):
    """inclusive [start, end] runs of a sorted position list"""
    if ones.size == 0:
        return np.zeros(0, U64), np.zeros(0, U64)
    cut = np.flatnonzero(np.diff(ones.astype(np.int64)) != 1)
    return ones[np.concatenate([[0], cut + 1])], ones[np.concatenate([cut, [ones.size - 1]])]


def words_of(c):
    bits = np.zeros(c.nblocks * B, np.uint8)
    bits[c.ones.astype(np.int64)] = 1
    return np.packbits(bits, bitorder="little").view(np.uint32)


DENSE_BLOCKS = 1024                              # up to here a case is imported from its words, above it is set run by run


def to_oracle(orc, c):
    """the case as a vector of the C port or of the reference build"""
    if c.nblocks <= DENSE_BLOCKS:
        return orc.import_words(words_of(c), True, c.nbits)
    v = orc.new(c.nbits)
    for s, e in zip(*runs_of(c.ones)):
        if s == e: v.set_bit(int(s))
        else: v.set_range(int(s), int(e))
    v.optimize()
    return v


# ---- the integer model of the build (bmx.hip: rs_tables .. rs_select_summary) ----
def sample_shape(nblocks):
    sh = 0
    while ((nblocks + (1 << sh) - 1) >> sh) > 2048: sh += 1
    return sh, (nblocks + (1 << sh) - 1) >> sh


def try16(nblocks, count, sel):
    return sel != 2 and float(nblocks) * 65536.0 / float(count) * 60.0 < 32768.0


def line_too_wide(ones, bits):
    """k_rs_sel_check: some line of K ones spans 2^bits bits or more"""
    K = 60 if bits == 16 else 30
    first = ones[::K]
    last = ones[np.minimum(np.arange(first.size) * K + K - 1, ones.size - 1)]
    return bool(((last - first) >= U64(1 << bits)).any())


def select_bits(c):
    sel = c.keys["rs_select_sel"]
    if not c.count or sel == 0: return 0
    for bits in ((16, 32) if try16(c.nblocks, c.count, sel) else (32,)):
        if not line_too_wide(c.ones, bits): return bits
    return 0


def has_lines(c):
    return c.keys["rs_lines"] == 2 and c.nblocks * RL_LINES < 0xFFFFFFFF


def sdir_shift_for(key, count, nlines):
    sh = key
    if key <= 0:
        want = 10.0 * float(count) / float(nlines)
        sh = 6
        while sh < 20 and float(1 << sh) * 1.4142 < want: sh += 1
    while ((count >> sh) + 2) * 4 > (8 << 20) and sh < 24: sh += 1
    return sh


def sdir_entries(count, sh):
    return ((count + (1 << sh) - 1) >> sh) + 1


def stop_shape(count, sdir_shift):
    ssh = sdir_shift
    while ((count + (1 << ssh) - 1) >> ssh) + 1 > STOP_ENTRIES and ssh < 40: ssh += 1
    return ssh, ((count + (1 << ssh) - 1) >> ssh) + 1


def line_of(pos):
    """global rank line and data bit inside it"""
    pos = np.asarray(pos, U64).astype(np.int64)
    off = pos & (B - 1)
    return (pos >> 16) * RL_LINES + off // RL_BITS, off % RL_BITS


def p8_table(c, ssh, n_top):
    k = np.arange(n_top, dtype=np.int64) << ssh
    live = k < c.count
    line, bit = line_of(c.ones[np.where(live, k, 0)])
    return np.where(live, 8 * line + bit // 120, 8 * (c.nblocks * RL_LINES - 1) + 7)


def group_spread(p8):
    n = p8.size
    g = np.arange(0, n, STOP_GROUP)
    return int((p8[np.minimum(g + STOP_GROUP - 1, n - 1)] - p8[g]).max())


def fb_of(spread):
    """the summary's fraction bits, or None where the summary is dropped"""
    fb = 3
    while fb > 0 and (spread >> (3 - fb)) > 65000: fb -= 1
    return None if (spread >> (3 - fb)) > 65000 else fb


class Summary:
    def __init__(self, c):
        self.sdir_shift = sdir_shift_for(c.keys["rs_sdir_shift"], c.count, c.nblocks * RL_LINES)
        self.entries = sdir_entries(c.count, self.sdir_shift)
        self.shift, self.n_top = stop_shape(c.count, self.sdir_shift)
        self.p8 = p8_table(c, self.shift, self.n_top)
        self.spread = group_spread(self.p8)
        self.fb = fb_of(self.spread) if c.nblocks * RL_LINES < (1 << 28) else None

    def first_guess(self, r):
        """entry_of (k_select_top): the bounds and the interpolated line of rank r -> (lo, hi, guess)"""
        idx0 = np.asarray(r, U64).astype(np.int64) - 1
        m = idx0 >> self.shift
        down = 3 - self.fb
        plo, phi = self.p8[m] >> down, self.p8[m + 1] >> down
        fr = idx0 & ((1 << self.shift) - 1)
        p2 = 2 * plo + 1 + ((2 * (phi - plo) * fr) >> self.shift)
        lo, hi = plo >> self.fb, phi >> self.fb
        return lo, hi, np.clip(p2 >> (self.fb + 1), lo, hi)


def expected_info(c):
    nb = max(c.nblocks, 1)
    by = nb * (4 + 8 + 8 + 256)
    lines = has_lines(c) and c.nblocks > 0
    if lines: by += nb * (RL_LINES * 128 + 16)
    if lines and c.count:
        s = Summary(c)
        by += s.entries * 4 + (STOP_BYTES if s.fb is not None else 0)
    bits = select_bits(c)
    sb = (c.count + (60 if bits == 16 else 30) - 1) // (60 if bits == 16 else 30) * SL_BYTES if bits else 0
    return {"bytes": by + sb, "has_lines": bool(lines), "select_offset_bits": bits, "select_lines_bytes": sb}


# ---- helpers of the constructions ----
def blk(b, offs):
    return (np.asarray(offs, np.int64) + int(b) * B).astype(U64)


def cat(parts):
    parts = [np.asarray(p, U64).ravel() for p in parts]
    return np.unique(np.concatenate(parts)) if parts else np.zeros(0, U64)


def at_line(line, bits):
    """global positions of data bits `bits` of global rank line `line`"""
    return blk(line // RL_LINES, (line % RL_LINES) * RL_BITS + np.asarray(bits, np.int64))


# ---- Grid A ----
A_CLASSES = "abcdefghijklmn"
SHORT_BATCHES = (1, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65)


def class_offsets(k):
    """the ones of a block class as offsets inside the block"""
    ar = np.arange
    f = np.concatenate([960 * ar(68), 960 * ar(68) + 959, [65280, 65535]])
    if k == "a": return ar(0)
    if k == "b": return ar(B)
    if k == "c": return np.array([0])
    if k == "d": return np.array([65535])
    if k == "e": return ar(65280, 65536)
    if k == "f": return np.sort(f)
    if k == "g": return np.unique(np.concatenate([f, ar(0, 2048, 2)]))
    if k == "h": return ar(65000, 65536)
    if k == "i": return ar(8192, 16384)
    if k == "j": return np.concatenate([[24576], ar(32768 - 32, 32768)])
    if k == "k": return np.concatenate([ar(0, 1274, 2), ar(1274, B)])       # 1,275 runs, the first of them ones
    if k == "l": return np.flatnonzero(np.random.default_rng(0xA11).integers(0, 2, B))
    if k == "m": return np.sort(np.concatenate([1024 * ar(1, 64) - 1, 1024 * ar(1, 64)]))
    if k == "n": return np.array([21823, 21824, 21825, 32735, 32736, 32737, 43647, 43648, 43649, 54559, 54560, 54561])
    raise KeyError(k)


def grid_a_layout():
    return A_CLASSES + A_CLASSES[::-1] + "o"


def grid_a(lines):
    lay = grid_a_layout()
    nbits = len(lay) * B - 777
    parts = [blk(b, class_offsets(k)) for b, k in enumerate(lay[:-1])]
    parts.append(np.array([(len(lay) - 1) * B + 5, nbits - 1], U64))       # class o: the partial last block
    c = Case("A.lines%d" % lines, nbits, cat(parts), {"rs_lines": lines, "rs_select_sel": 1}, batches=SHORT_BATCHES)
    c.rank_q = np.concatenate([np.arange(nbits, dtype=U64), dead_positions(c)])
    return c


def grid_a_derived(c):
    """the constructed list of the derived queries: (left, right) of count_range, positions of rank_corrected / count_to_test,
    (rank, from) of find_rank -- incl. left > right, from past the end, rank 0"""
    o, n = c.ones.astype(np.int64), c.nbits
    pick = o[:: max(1, o.size // 97)]
    left = np.concatenate([pick, pick + 1, [0, 0, n - 1, 70000, n - 1, B, B - 1]])
    right = np.concatenate([pick + 960, pick, [0, n - 1, n - 1, 3, 0, 2 * B - 1, B]])
    right = np.minimum(right, n - 1); left = np.minimum(left, n - 1)
    posn = np.minimum(np.concatenate([pick, pick + 1, pick - 1 + (pick == 0), [0, n - 1, B - 1, B]]), n - 1)
    rank = np.concatenate([np.ones(pick.size, np.int64), np.arange(pick.size) % 5, [0, 1, c.count, c.count + 1, 1, 1, 3]])
    frm = np.concatenate([pick, pick + 1, [0, 0, 0, 0, n - 1, n + 5, n - 1]])
    return {"left": left.astype(U64), "right": right.astype(U64), "pos": posn.astype(U64), "rank": rank.astype(U64), "from": frm.astype(U64)}


# ---- Grid B ----
B1_X = (1, 40000, 65535)
B1_LAST = ("x-1", "x", "b+2")                  # span 65,535 | 65,536 | the last one two blocks on, the block between NULL
B1_PLACE = ("first", "middle", "last59", "last2")
B1_CLAIM = {"x-1": 16, "x": 32, "b+2": 32}


def b1_case(x, last, place):
    n = {"last59": 59, "last2": 2}.get(place, 60)
    pre = 0 if place == "first" else 20 * 60
    post = 0 if place.startswith("last") else 20 * 60
    if place == "first": post *= 2
    if place.startswith("last"): pre *= 2
    first = 1 * B + x
    end = {"x-1": 2 * B + x - 1, "x": 2 * B + x, "b+2": 3 * B + 7 + n}[last]
    crit = np.concatenate([[first], np.arange(end - (n - 2), end), [end]]).astype(U64)
    return Case("B1.x%d.%s.%s" % (x, last, place), 5 * B, cat([np.arange(pre), crit, 4 * B + 11 + np.arange(post)]),
                {"rs_select_sel": 1}, claims={"select_offset_bits": B1_CLAIM[last]})


def grid_b1(x):
    cs = [b1_case(x, last, place) for last in B1_LAST for place in B1_PLACE]
    cs.append(Case("B1.x%d.last1" % x, 5 * B, cat([np.arange(40 * 60), [2 * B + x]]), {"rs_select_sel": 1}, claims={"select_offset_bits": 16}))
    return cs


B2_COUNTS = {1: (1, 59, 60, 61, 119, 120, 121), 2: (1, 29, 30, 31, 59, 60, 61)}


def grid_b2():
    return [Case("B2.sel%d.n%d" % (sel, n), B - 100, 7 * np.arange(n) + 3, {"rs_select_sel": sel}) for sel in (1, 2) for n in B2_COUNTS[sel]]


B3_ROWS = {1: (4095, 4096, 4097, 8192), 2: (2047, 2048, 2049)}


def row_offsets(n):
    """n ones inside one 8,192-bit row: the even bits first, then the odd ones"""
    return np.sort(np.concatenate([2 * np.arange(min(n, 4096)), 2 * np.arange(max(n - 4096, 0)) + 1]))


def grid_b3():
    cs = []
    for sel in (1, 2):
        for n in B3_ROWS[sel]:
            for lead in (1, 2):                                              # the block's first one has an odd / an even global number
                ones = cat([blk(0, 60000 + 3 * np.arange(lead)), blk(1, 2 * 8192 + row_offsets(n)), blk(1, 5 * 8192 + 2 * np.arange(4096))])
                cs.append(Case("B3.sel%d.row%d.lead%d" % (sel, n, lead), 2 * B, ones, {"rs_select_sel": sel}, claims={"select_offset_bits": 16 * sel}))
    return cs


def grid_b4():
    nbits = 16 * B
    return [Case("B4.n%d" % n, nbits, (np.arange(n, dtype=np.int64) * nbits) // n, {"rs_select_sel": 1},
                 claims={"select_offset_bits": 16 if n > 1920 else 32}) for n in (1919, 1920, 1921)]


def grid_b5():
    nb = 65538
    edge = 1 << 32
    straddle = cat([np.arange(0, 600, 5), edge - 3000 + 211 * np.arange(14), edge + 97 * np.arange(16), blk(nb - 1, [0, 65535])])
    far = cat([np.arange(0, 100, 2), blk(nb - 1, 64 + 3 * np.arange(45))])          # ones 30 .. 59: twenty in block 0, ten in the last block
    cs = [Case("B5.straddle", nb * B, straddle, {"rs_select_sel": 1}, claims={"select_offset_bits": 32}),
          Case("B5.far", nb * B, far, {"rs_select_sel": 1}, claims={"select_offset_bits": 0})]
    for c in cs:
        c.rank_q = np.concatenate([around(c, c.ones), np.array([edge - 1, edge, edge + 1], U64), dead_positions(c)])
    return cs


# ---- Grid C ----
KEYS_C = {"rs_lines": 2, "rs_select_sel": 0, "rs_sdir_shift": 6, "rs_select_top": 1}
C3_ENTRIES = 1000
C3_BATCHES = (1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 1023, 1024, 1025, 64 * C3_ENTRIES)


def c1_case(s, count, place):
    """ones numbered m 2^s (the sampled ones) first of their line | last of their line | alone in a line behind three empty ones;
    the ones between two samples fill the following line(s) from its first bit"""
    S, parts, line = 1 << s, [], 0
    for m in range((count + S - 1) // S):
        n = min(S, count - m * S)                                            # ones of this entry, the sampled one first
        if place == "first":
            parts.append(at_line(line, np.arange(min(n, 200)))); used = min(n, 200)
        elif place == "last":
            parts.append(at_line(line, [959] if (line % RL_LINES) < 68 else [255])); used = 1
        else:
            line += 3; parts.append(at_line(line, [400 % (960 if (line % RL_LINES) < 68 else 256)])); used = 1
        line += 1
        while used < n:                                                      # the rest: whole lines of up to 200 ones
            k = min(n - used, 200)
            parts.append(at_line(line, np.arange(k))); used += k; line += 1
    nblocks = (line + RL_LINES - 1) // RL_LINES + 1
    keys = dict(KEYS_C); keys["rs_sdir_shift"] = s
    return Case("C1.s%d.n%d.%s" % (s, count, place), nblocks * B - 31, cat(parts), keys)


def grid_c1():
    return [c1_case(s, n, place) for s in (6, 8) for n in ((1 << s) - 1, 1 << s, (1 << s) + 1, 3 << s, (3 << s) + 1) for place in ("first", "last", "alone")]


C2_SPANS = (1, 2, 5, 9, 100, 5000)


def c2_case(L, mirror):
    """entries of 64 ones; the skewed entry spans L lines: its sampled one first of the entry's line, ones 1 .. 62 in the line just
    before the next entry's line (mirror: in the entry's own line), one 63 in the next entry's line with that entry's sample"""
    parts, line = [], 0
    def ordinary(n):
        nonlocal line
        for _ in range(n):
            parts.append(at_line(line, 15 * np.arange(64) % 256 if (line % RL_LINES) == 68 else 15 * np.arange(64))); line += 1
    ordinary(3)
    wide = 960 if (line % RL_LINES) < 68 else 256
    near = line if mirror or L == 1 else line + L - 1
    w2 = 960 if (near % RL_LINES) < 68 else 256
    parts.append(at_line(line, [0]))
    parts.append(at_line(near, (1 if near == line else 0) + np.arange(62) * ((w2 - 2) // 62)))
    line += L
    parts.append(at_line(line, [0])); parts.append(at_line(line, 2 + np.arange(64))); line += 1          # one 63 of the skewed entry + a whole entry
    ordinary(3)
    nblocks = (line + RL_LINES - 1) // RL_LINES
    return Case("C2.L%d.%s" % (L, "own" if mirror else "far"), nblocks * B, cat(parts), KEYS_C)


def grid_c2():
    return [c2_case(L, mirror) for L in C2_SPANS for mirror in (False, True)]


def grid_c3():
    parts = []
    for m in range(C3_ENTRIES):
        parts.append(at_line(10 * m, [0])); parts.append(at_line(10 * m + 8, np.arange(63)))
    nblocks = (10 * C3_ENTRIES + RL_LINES - 1) // RL_LINES
    c = Case("C3", nblocks * B, cat(parts), KEYS_C, batches=C3_BATCHES, claims={"fb": 3, "miss_share": 0.75, "nblocks": 145})
    c.select_r = np.concatenate([np.random.default_rng(0xC3).permutation(np.arange(1, c.count + 1, dtype=U64)), dead_ranks(c)])
    c.rank_q = np.concatenate([around(c, c.ones), dead_positions(c)])
    return [c]


C4_SPREADS = ((65000, 3), (65001, 2), (130001, 2), (130002, 1), (260003, 1), (260004, 0), (520007, 0), (520008, None))


def grid_c4():
    cs = []
    for spread, fb in C4_SPREADS:
        line, bit = spread // 8, 120 * (spread % 8)
        nblocks = line // RL_LINES + 1
        c = Case("C4.spread%d" % spread, nblocks * B, cat([np.arange(4032), at_line(line, bit + np.arange(69))]), KEYS_C,
                 claims={"fb": fb, "spread": spread})
        c.rank_q = np.concatenate([around(c, c.ones), dead_positions(c)])
        cs.append(c)
    return cs


def grid_c5():
    cs = []
    for extra in (0, 1):
        n = 63 * B + 65472 + extra
        c = Case("C5.n%d" % n, 64 * B, np.arange(n), KEYS_C, claims={"stop_shift": 6 + extra})
        c.select_r = np.concatenate([np.arange(1, 201), np.arange(1, n + 1, 97), np.arange(n - 199, n + 1), dead_ranks(c)]).astype(U64)
        c.rank_q = np.concatenate([c.ones[::4099], around(c, [63 * B, n - 1]), dead_positions(c)])
        cs.append(c)
    return cs


# ---- Grid D ----
D_NBLOCKS = (1, 31, 32, 33, 2048, 2049, 4096, 4097, 16384, 16385, 65537, 131073)
D_LINES_MAX = 4097
GAP3 = (0, 30000, 65535)


def d_carriers(nb):
    sh, ns = sample_shape(nb)
    G, g = 1 << sh, ns // 2
    want = [0, nb - 1, g * G, g * G + G - 1, (g + 1) * G + 31, (g + 1) * G + 32, (g + 1) * G + 33, (g + 2) * G + 2, (g + 2) * G + 43, 16383, 16384,
            31, 32, 33, 5 * 64 + 2, 5 * 64 + 43]
    return sorted({b for b in want if 0 <= b < nb})


def d_case(nb, lines):
    car = d_carriers(nb)
    parts = [blk(b, np.arange(B) if i % 3 == 1 else GAP3) for i, b in enumerate(car)]
    c = Case("D.n%d.lines%d" % (nb, lines), nb * B, cat(parts), {"rs_lines": lines, "rs_select_sel": 0, "rs_select_top": 1},
             claims={"sample_shift": sample_shape(nb)[0]})
    borders = np.array([x for b in car for x in (b * B - 1, b * B, b * B + B - 1, b * B + B) if 0 <= x < c.nbits], U64)
    c.rank_q = np.concatenate([around(c, c.ones), borders, dead_positions(c)])
    return c


# ---- the chunks the tests are parametrised by ----
def chunks():
    ch = {"A.lines0": lambda: [grid_a(0)], "A.lines2": lambda: [grid_a(2)]}
    for x in B1_X: ch["B1.x%d" % x] = (lambda x=x: grid_b1(x))
    ch.update({"B2": grid_b2, "B3": grid_b3, "B4": grid_b4, "B5": grid_b5, "C1": grid_c1, "C2": grid_c2, "C3": grid_c3, "C4": grid_c4, "C5": grid_c5})
    for nb in D_NBLOCKS:
        ch["D.n%d.lines0" % nb] = (lambda nb=nb: [d_case(nb, 0)])
        if nb <= D_LINES_MAX: ch["D.n%d.lines2" % nb] = (lambda nb=nb: [d_case(nb, 2)])
    return ch


# ---- the fixture: what an oracle (the reference build, or the C port) answers ----
def _literals(a):
    a = np.asarray(a)
    return [int(x) for x in a[np.linspace(0, a.size - 1, min(6, a.size)).astype(np.int64)]] if a.size else []


def oracle_entry(orc, c):
    v = to_oracle(orc, c)
    rs = orc.rs_build(v)
    bc, sub = rs.export(c.nblocks)
    bc = np.concatenate([bc, np.zeros(c.nblocks - bc.size, np.uint32)]); sub = np.concatenate([sub, np.zeros(c.nblocks - sub.size, U64)])
    q, r = c.ref_rank_q(), c.ref_select_r()
    ra = rs.rank(q)
    pos, found = rs.select(r)
    pos = np.where(found, pos, U64(0))
    e = {"count": int(v.count()), "bcount": sha(bc, np.uint32), "sub_count": sha(sub), "rank": sha(ra), "select": sha(np.concatenate([pos, found.astype(U64)])),
         "rank_at": _literals(ra), "select_at": _literals(pos)}
    if c.name.startswith("A."):
        d = grid_a_derived(c)
        cr = [rs.count_range(int(l), int(r_)) for l, r_ in zip(d["left"], d["right"])]
        rc = [rs.rank_corrected(int(n)) for n in d["pos"]]
        ct = [rs.count_to_test(int(n)) for n in d["pos"]]
        fr = [rs.find_rank(int(k), int(f)) for k, f in zip(d["rank"], d["from"])]
        e["derived"] = {"count_range": sha(cr), "rank_corrected": sha(rc), "count_to_test": sha(ct),
                        "find_rank": sha([p if f else 0 for f, p in fr] + [int(f) for f, _ in fr])}
    return e


def oracle_fixture(orc, only=None):
    out = {}
    for name, make in chunks().items():
        if only is not None and name not in only: continue
        for c in make():
            if c.fits_reference(): out[c.name] = oracle_entry(orc, c)
    return {"cases": out}


def model_entry(c):
    """the same entry from the closed forms alone (no export hashes: the block tables are the oracle's)"""
    q, r = c.ref_rank_q(), c.ref_select_r()
    ra = rank_expect(c, q)
    found, pos = select_expect(c, r)
    e = {"count": c.count, "rank": sha(ra), "select": sha(np.concatenate([pos, found.astype(U64)])), "rank_at": _literals(ra), "select_at": _literals(pos)}
    if c.name.startswith("A."):
        d = grid_a_derived(c)
        rk, bit = rank_expect(c, d["pos"]), bit_expect(c, d["pos"])
        f, p = find_rank_expect(c, d["rank"], d["from"])
        e["derived"] = {"count_range": sha(count_range_expect(c, d["left"], d["right"])), "rank_corrected": sha(rk - bit.astype(U64)),
                        "count_to_test": sha(np.where(bit, rk, U64(0))), "find_rank": sha(np.concatenate([p, f.astype(U64)]))}
    return e
