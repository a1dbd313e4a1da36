"""Constructed cases for the pairwise path (bit_and / or / xor / sub, count_*, op2_async; tests/test_pair_host.py,
tests/test_gpu_pair.py): two operands over the same block columns, every column one cell (class of A, class of B) whose
blocks are given by construction, so that `A op B` is a closed form in NumPy and the KIND the reference stores for the
result column follows from a restatement of its rule (model_kind below, written from combine_operation_block_*,
clone_assign_block, clone_gap_block and optimize_bit_block of the reference -- not from the kernels' op2_store_mode).

  Grid K   every ordered pair of 18 block classes: empty, full, short / long / limit-length run lists, complements,
           disjoint and nested partners, random words.  These are the cells on which the storage rule branches.
  Grid L   one GAP operand per run-list length at every border of the GAP header's levels, of the 16-byte chunks of
           a run list and of the 512-run decode rounds, against zero / ones / random / a GAP block.
A pair is imported optimised (kinds by content) or raw (every block a bit-block); the short form holds the case columns
only, the long form appends filler up to N blocks (ragged: the longer operand ends in 13 columns of Grid-K classes).
No GPU, no oracle: pure NumPy."""
import hashlib

import numpy as np

from and_fold_cases import MAX_GAP_LEN, block_of, block_of_ends, gap_words, len_sbit, words_of

B = 65536
BW = 2048
NULL, FULL, BIT, GAP = 0, 1, 2, 3
AND, OR, XOR, SUB = 0, 1, 2, 3
OPS = (AND, OR, XOR, SUB)
OP_NAMES = ("and", "or", "xor", "sub")
FLAVOURS = ((True, True), (True, False), (False, True), (False, False))          # (A optimised, B optimised)
L_LENS = (2, 3, 7, 8, 9, 15, 16, 17, 124, 125, 252, 253, 503, 504, 505, 508, 509, 511, 512, 513, 1015, 1016, 1017, 1023, 1024,
          1025, 1274, 1275)
L_PARTNERS = ("zero", "ones", "d", "gA")
LONG_N = (2048, 2049, 3073, 4097)
RAGGED = ((2048, 2061), (2061, 2048))
FIXTURE_N = 2049
CUT = 77                                   # the partial-block pairs end 77 bits before a block border


def flavour_name(fl):
    return "%s,%s" % tuple("opt" if o else "raw" for o in fl)


# ---------------------------------------------------------------------------------------------------------------------
# block classes
# ---------------------------------------------------------------------------------------------------------------------
def _runs_block(n_one_runs, first, last, start, stride, width):
    """n 1-runs of `width` bits at `stride` from `start`; first / last: bit 0 / bit 65535 belongs to the first / last of them"""
    runs = [(start + stride * k, start + stride * k + width - 1) for k in range(n_one_runs)]
    if first: runs[0] = (0, runs[0][1])
    if last: runs[-1] = (runs[-1][0], B - 1)
    return block_of(runs)


def block_with_len(ln, sbit):
    k = np.arange(1, ln)
    return block_of_ends(np.concatenate([30 + 50 * k + (k * 7) % 13, [B - 1]]), sbit)


def _classes():
    c = {}
    c["zero"] = np.zeros(B, bool)
    c["ones"] = np.ones(B, bool)
    c["g2_0"] = block_of([(30000, B - 1)])
    c["g2_1"] = block_of([(0, 40000)])
    c["gA"] = _runs_block(350, False, False, 100, 90, 40)           # 701 runs: bits 100 + 90 k .. + 39
    c["nA"] = ~c["gA"]
    c["gB"] = _runs_block(350, False, False, 150, 90, 20)           # in the holes of gA, never adjacent to it
    c["gS"] = _runs_block(175, False, False, 105, 180, 16)          # inside every other run of gA
    c["g1275_0"] = block_with_len(MAX_GAP_LEN, 0)
    c["g1275_1"] = block_with_len(MAX_GAP_LEN, 1)
    c["g1276"] = block_with_len(MAX_GAP_LEN + 1, 0)
    # gh and its partners.  A block of n 1-runs has 2 n + 1 - s - e runs (s, e: its first and its last bit).  The three
    # hold pairwise disjoint, never adjacent 1-runs (gh at 0 mod 100, the partners at 50 mod 100), so OR == XOR and the
    # 1-runs add up:   gh  320 1-runs, s = 1, e = 0 -> 640 runs;   gh1 318, s = 0, e = 1 -> 636;   gh2 318, s = 0, e = 0 -> 637
    #   gh | gh1: 638 1-runs, s = 1, e = 1 -> 2 * 638 + 1 - 2 = 1275 runs      gh | gh2: 638, s = 1, e = 0 -> 1276 runs
    c["gh"] = _runs_block(320, True, False, 0, 100, 10)
    c["gh1"] = _runs_block(317, False, False, 50, 100, 10) | block_of([(40000, B - 1)])
    c["gh2"] = _runs_block(317, False, False, 50, 100, 10) | block_of([(40000, 40009)])
    rng = np.random.default_rng(20261)
    d = rng.integers(0, 2, B).astype(bool)
    c["d"] = d
    c["nd"] = ~d
    c["dS"] = d & rng.integers(0, 2, B).astype(bool)
    c["dfew"] = block_of([(20000, 29999)])
    return c


def l_block(ln, sbit):
    """ln runs, the first of value sbit.  Word j of the run list (j >= 1) is the end of run j.  Word 1 = 0: block bit 0 is a run
    of its own; word len = 65535 = word len - 1 + 1: bit 65534 ends a run (len >= 3); word m = word m - 1 + 1 for every m that
    is a multiple of 8: the one-bit run m starts in the last word of one 16-byte chunk and ends in the first of the next
    (words 511 / 512 and 1,023 / 1,024 among them); the other runs are 40 .. 50 bits, the slack sits in run 2."""
    if ln == 2:
        return block_of_ends([0, B - 1], sbit)
    j = np.arange(2, ln + 1)
    inc = 40 + (j * 7) % 11
    inc[j % 8 == 0] = 1
    inc[-1] = 1
    inc[0] += (B - 1) - int(inc.sum())
    ends = np.concatenate([[0], np.cumsum(inc)])
    assert ends[-1] == B - 1 and inc[0] > 0
    return block_of_ends(ends, sbit)


_BITS = _classes()
K_NAMES = tuple(_BITS)
for _ln in L_LENS:
    for _sb in (0, 1):
        _BITS["L%d.%d" % (_ln, _sb)] = l_block(_ln, _sb)
WORDS = {n: words_of(b) for n, b in _BITS.items()}
RUNS = {n: len_sbit(b) for n, b in _BITS.items()}                   # name -> (runs, first bit)
FILL_CYCLE = ("zero", "ones", "gA", "d")


def class_bits(name):
    return _BITS[name]


def k_columns():
    return [(a, b) for a in K_NAMES for b in K_NAMES]


def l_columns():
    return [("L%d.%d" % (ln, sb), p) for ln in L_LENS for sb in (0, 1) for p in L_PARTNERS]


def case_columns():
    return k_columns() + l_columns()


# ---------------------------------------------------------------------------------------------------------------------
# words -> per-block facts (vectorised: the long forms hold 4,097 blocks)
# ---------------------------------------------------------------------------------------------------------------------
def pad_blocks(words):
    n = (-words.size) % BW
    return np.concatenate([words, np.zeros(n, np.uint32)]) if n else words


def block_facts(words):
    """(runs, first bit, popcount) of every block of a word array"""
    w = pad_blocks(np.ascontiguousarray(words, np.uint32)).reshape(-1, BW)
    nxt = np.empty_like(w)
    nxt[:, :-1] = w[:, 1:] & 1
    nxt[:, -1] = w[:, -1] >> 31                                      # (no transition behind bit 65535)
    t = w ^ ((w >> 1) | (nxt << 31))
    return (1 + np.bitwise_count(t).sum(axis=1, dtype=np.int64), (w[:, 0] & 1).astype(np.int64),
            np.bitwise_count(w).sum(axis=1, dtype=np.int64))


def popcount(words):
    return int(np.bitwise_count(words).sum(dtype=np.int64))


def import_kinds(words, optimised):
    """bit_import_u32: a bit-block per 2,048 words; with optimize, optimize_bit_block -- one run -> NULL / FULL, fewer than 1,276
    runs -> GAP (src/bmbvimport.h:46, src/bmblocks.h:1414)"""
    runs, first, _ = block_facts(words)
    if not optimised:
        return np.full(runs.size, BIT, np.int64)
    return np.where(runs == 1, np.where(first == 1, FULL, NULL), np.where(runs <= MAX_GAP_LEN, GAP, BIT))


def apply_op(op, a, b):
    n = max(a.size, b.size)
    a = np.concatenate([a, np.zeros(n - a.size, np.uint32)]) if a.size < n else a
    b = np.concatenate([b, np.zeros(n - b.size, np.uint32)]) if b.size < n else b
    return a & b if op == AND else a | b if op == OR else a ^ b if op == XOR else a & ~b


# ---------------------------------------------------------------------------------------------------------------------
# the reference's storage rule, restated from its source
# ---------------------------------------------------------------------------------------------------------------------
def _cloned(k, runs, first, invert=False):
    """blocks_manager::clone_assign_block (src/bmblocks.h:894): a GAP block of one run becomes NULL / FULL, any other GAP block stays
    one (inverted: the same run list), a bit-block stays a bit-block whatever it holds.  clone_gap_block(gap_block, gap_res) (:838)
    asks gap_calc_level for gap_length = runs + 1 words: the GAP block of GAP_RESULT_MAX runs, which only a GAP x GAP result can be,
    does not pass and is copied as a bit-block"""
    if k == NULL: return FULL if invert else NULL
    if k == FULL: return NULL if invert else FULL
    if k == GAP and runs == 1: return FULL if (first ^ invert) else NULL
    if k == GAP and runs + 1 > GAP_LEVEL_MAX: return BIT
    return k


GAP_LEVEL_MAX = 1276                        # gap_calc_level (src/bmfunc.h:5418): len <= glevel_len[3] - 4 is the last GAP level
GAP_RESULT_MAX = GAP_LEVEL_MAX              # the longest GAP x GAP result kept as a GAP block: ONE run more than an import keeps


def _gap_result(runs, first):
    """clone_gap_block(i, j, buf, len) (src/bmblocks.h:865) with len = the result's run count: an all-zero result is not stored; one
    that no GAP level holds (gap_calc_level(len) < 0: more than 1,276 runs) becomes a bit-block; anything else is a GAP block,
    the all-ones result of one run included.  (optimize_bit_block and the importer compare runs < 1,276: their limit is 1,275.)"""
    if runs == 1 and not first: return NULL
    return GAP if runs <= GAP_RESULT_MAX else BIT


def _computed(runs, first, compress):
    """a bit-block the operation reports as "optimization may be needed": bit_and / or / xor / sub run optimize_bit_block on it
    under opt_compress only (src/bm.h:6052, src/bmblocks.h:1414)"""
    if not compress: return BIT
    if runs == 1: return FULL if first else NULL
    return GAP if runs < MAX_GAP_LEN + 1 else BIT


def model_kind(op, compress, ka, a, kb, b, r):
    """kind of the result block.  a, b, r: (runs, first bit) of the two operand blocks and of a op b"""
    zero, one = r == (1, 0), r == (1, 1)
    if op == AND:                                           # combine_operation_block_and, src/bm.h:7100
        if ka == NULL or kb == NULL: return NULL
        if ka == FULL: return _cloned(kb, *b)
        if kb == FULL: return _cloned(ka, *a)
        if ka == GAP and kb == GAP: return _gap_result(*r)
        return NULL if zero else _computed(*r, compress)    # (GAP x bit: bit_is_all_zero; bit x bit: the digest)
    if op == OR:                                            # :6945
        if ka == NULL: return _cloned(kb, *b)
        if kb == NULL: return _cloned(ka, *a)
        if ka == FULL or kb == FULL: return FULL
        if ka == GAP and kb == GAP: return _gap_result(*r)
        if ka == GAP or kb == GAP: return _computed(*r, compress)          # (no test: all ones stays a bit-block)
        return FULL if one else _computed(*r, compress)     # (bit_block_or_2way reports all ones)
    if op == XOR:                                           # :7018
        if ka == NULL: return _cloned(kb, *b)
        if kb == NULL: return _cloned(ka, *a)
        if ka == FULL: return _cloned(kb, *b, invert=True)
        if kb == FULL: return _cloned(ka, *a, invert=True)
        if ka == GAP and kb == GAP: return _gap_result(*r)
        if ka == GAP or kb == GAP: return _computed(*r, compress)
        return NULL if zero else _computed(*r, compress)
    if ka == NULL or kb == FULL: return NULL                # combine_operation_block_sub, :7285
    if kb == NULL: return _cloned(ka, *a)
    if ka == GAP and kb == GAP: return _gap_result(*r)      # (a FULL first operand is the real all-ones bit-block from here on)
    if kb == GAP: return _computed(*r, compress)            # bit - GAP: a copy with the runs cleared, not tested
    return NULL if zero else _computed(*r, compress)        # GAP - bit, bit - bit: the accumulated OR / the digest


def model_kinds(op, compress, ka, fa, kb, fb, fr):
    """per column; ka / kb: kinds of the operands (missing columns of the shorter one: NULL), f*: block_facts of a, b and a op b"""
    n = fr[0].size
    out = np.zeros(n, np.int64)

    def at(k, f, c):
        return (int(k[c]), (int(f[0][c]), int(f[1][c]))) if c < k.size else (NULL, (1, 0))
    for c in range(n):
        (xa, a), (xb, b) = at(ka, fa, c), at(kb, fb, c)
        out[c] = model_kind(op, compress, xa, a, xb, b, (int(fr[0][c]), int(fr[1][c])))
    return out


def kinds_str(kinds):
    """the kinds of a vector as one string of hexadecimal digits, two blocks per digit (4 * kind of the even block + kind of the
    odd one; a last odd block is paired with 0)"""
    k = np.asarray(kinds, np.int64)
    if k.size & 1: k = np.concatenate([k, [0]])
    return "".join("%x" % x for x in (4 * k[0::2] + k[1::2]))


def kinds_of_str(s, nblocks):
    k = np.array([int(ch, 16) for ch in s], np.int64)
    return np.stack([k >> 2, k & 3], axis=1).ravel()[:nblocks]


def sha(words):
    return hashlib.sha256(np.ascontiguousarray(words, np.uint32).tobytes()).hexdigest()


# ---------------------------------------------------------------------------------------------------------------------
# case pairs
# ---------------------------------------------------------------------------------------------------------------------
def _raw_filler(seed, nblocks):
    """seeded words of 30 % ones"""
    rng = np.random.default_rng(seed)
    out = np.empty(nblocks * BW, np.uint32)
    for lo in range(0, nblocks, 256):
        n = min(256, nblocks - lo)
        bits = rng.random(n * B, np.float32) < np.float32(0.3)
        out[lo * BW:(lo + n) * BW] = np.packbits(bits, bitorder="little").view(np.uint32)
    return out


class Pair:
    """two operands: cols[c] = (class of A, class of B) names the case columns; what follows them depends on how the operand is
    imported (optimised: a cycle of zero / ones / gA / d, all 16 cell pairs; raw: seeded 30 % words)"""

    def __init__(self, name, cols, na=None, nb=None, tail_a=(), tail_b=(), cut=0):
        self.name, self.cols, self.cut = name, list(cols), cut
        self.n = (len(self.cols) if na is None else na, len(self.cols) if nb is None else nb)
        self.tails = (list(tail_a), list(tail_b))
        self._w = {}
        assert min(self.n) >= len(self.cols) and (not cut or self.n[0] == self.n[1])

    def __repr__(self):
        return "pair %s (%d x %d blocks%s)" % (self.name, self.n[0], self.n[1], ", cut %d" % self.cut if self.cut else "")

    @property
    def nblocks(self):
        return max(self.n)

    @property
    def nbits(self):
        return self.nblocks * B - self.cut

    def filler_names(self, side, n):
        k = np.arange(n)
        idx = k % 4 if side == 0 else (k // 4) % 4
        return [FILL_CYCLE[i] for i in idx]

    def names(self, side, optimised):
        """class name per column of one operand (None: a column of raw filler)"""
        head = [c[side] for c in self.cols]
        tail = self.tails[side]
        nfill = self.n[side] - len(head) - len(tail)
        return head + (self.filler_names(side, nfill) if optimised else [None] * nfill) + tail

    def words(self, side, optimised):
        has_filler = self.n[side] > len(self.cols) + len(self.tails[side])
        key = (side, optimised if has_filler else True)             # (without filler both flavours import the same words)
        if key not in self._w:
            names = self.names(side, optimised)
            w = np.empty(len(names) * BW, np.uint32)
            nfill = sum(1 for x in names if x is None)
            fill = _raw_filler(977 + side, nfill) if nfill else None
            at = len(self.cols)
            for c, x in enumerate(names):
                if x is not None: w[c * BW:(c + 1) * BW] = WORDS[x]
            if nfill: w[at * BW:(at + nfill) * BW] = fill
            if self.cut:
                assert self.cut < 96 and not w[-3:].any()               # (the cut removes nothing)
            w.setflags(write=False)
            self._w[key] = w
        return self._w[key]

    def cell(self, col, fl=(True, True)):
        """what column col holds, for a failure message"""
        if col < len(self.cols):
            grid = "Grid L" if self.cols[col][0].startswith("L") else "Grid K"
            return "%s, column %d = (%s, %s)" % (grid, col, *self.cols[col])
        return "column %d = (%s, %s)" % (col, *[(self.names(s, fl[s]) + ["missing"] * self.nblocks)[col] or "raw filler" for s in (0, 1)])


class Expect:
    """closed form of one operation over a pair in one flavour: words and count from the construction, kinds from model_kind"""

    def __init__(self, pair, fl, swap=False):
        self.pair, self.fl, self.swap = pair, fl, swap
        self.w = [pair.words(0, fl[0]), pair.words(1, fl[1])]
        self.facts = [block_facts(w) for w in self.w]
        self.kinds = [import_kinds(w, o) for w, o in zip(self.w, fl)]
        if swap:
            self.w.reverse(); self.facts.reverse(); self.kinds.reverse()
        self._r, self._c = {}, None

    def __repr__(self):
        return "%r %s%s" % (self.pair, flavour_name(self.fl), " (B, A)" if self.swap else "")

    def result(self, op):
        """(words, facts, count) of a op b"""
        if op not in self._r:
            r = apply_op(op, self.w[0], self.w[1])
            f = block_facts(r)
            self._r = {op: (r, f, int(f[2].sum()))}                     # (one operation is kept: 32 MiB each at 4,097 blocks)
        return self._r[op]

    def count(self, op):
        return self.counts()[op]

    def counts(self):
        """the four counts (AND, OR, XOR, SUB) from one pass: |a & b| and the two operands' own counts"""
        if self._c is None:
            n = min(self.w[0].size, self.w[1].size)
            c_and, ca, cb = popcount(self.w[0][:n] & self.w[1][:n]), int(self.facts[0][2].sum()), int(self.facts[1][2].sum())
            self._c = (c_and, ca + cb - c_and, ca + cb - 2 * c_and, ca - c_and)
        return self._c

    def result_kinds(self, op, compress):
        return model_kinds(op, compress, self.kinds[0], self.facts[0], self.kinds[1], self.facts[1], self.result(op)[1])

    def cell(self, col):
        p = self.pair
        s = p.cell(col, self.fl)
        return s + (" -- operands swapped" if self.swap else "")


def first_diff(e, got_words=None, want_words=None, got_kinds=None, want_kinds=None):
    """names the first column in which two results differ"""
    if got_words is not None:
        bad = np.flatnonzero(got_words != want_words)
        if bad.size: return "words differ in %s" % e.cell(int(bad[0]) // BW)
    if got_kinds is not None:
        g, w = np.asarray(got_kinds), np.asarray(want_kinds)
        if g.size != w.size: return "kinds: %d blocks, expected %d" % (g.size, w.size)
        bad = np.flatnonzero(g != w)
        if bad.size: return "kind %d, expected %d in %s" % (g[bad[0]], w[bad[0]], e.cell(int(bad[0])))
    return None


_PAIRS = {}


def _pair(key, make):
    if key not in _PAIRS:
        _PAIRS[key] = make()
    return _PAIRS[key]


def short_pair():
    return _pair("short", lambda: Pair("short", case_columns()))


def long_pair(n):
    return _pair(("long", n), lambda: Pair("long%d" % n, case_columns(), n, n))


def ragged_pair(na, nb):
    """the last 13 columns of the longer operand cycle through the Grid-K classes: x op missing"""
    tail = [K_NAMES[(5 * k + 2) % len(K_NAMES)] for k in range(13)]
    return _pair(("ragged", na, nb), lambda: Pair("ragged%dx%d" % (na, nb), case_columns(), na, nb, tail if na > nb else (), tail if nb > na else ()))


def cut_pair():
    """nbits = N * 65536 - 77: the case columns and one more column of (g2_1, dfew), blocks that hold nothing in their last 77 bits"""
    return _pair("cut", lambda: Pair("cut", case_columns(), len(case_columns()) + 1, len(case_columns()) + 1, ["g2_1"], ["dfew"], CUT))


# ---------------------------------------------------------------------------------------------------------------------
# the chain: first-level results hold one-run GAP blocks, all-zero bit-blocks and FULL blocks that no import produces
# ---------------------------------------------------------------------------------------------------------------------
CHAIN_FIRST = (OR, XOR)                                     # R = A | B, R' = A ^ B of the (opt, opt) short form
# (the last three copy every block of R -- as it is, as it is, inverted: the one-run GAP block becomes FULL / NULL, the all-zero
# bit-block stays, the GAP block of 1,276 runs becomes a bit-block; 0 / 1: a vector of NULL / of FULL blocks only)
CHAIN_LINKS = (("R&A", AND, "R", "A"), ("R^B", XOR, "R", "B"), ("R-A", SUB, "R", "A"), ("A-R", SUB, "A", "R"), ("R|R'", OR, "R", "R'"),
               ("R|0", OR, "R", "0"), ("1&R", AND, "1", "R"), ("R^1", XOR, "R", "1"))


def chain_names():
    """every second-level result: (first-level op that made R, link name)"""
    return [(OP_NAMES[f], link[0]) for f in CHAIN_FIRST for link in CHAIN_LINKS]


def chain_constants():
    """words of the vectors 0 and 1 of the chain, as long as the short form"""
    n = len(case_columns()) * BW
    return np.zeros(n, np.uint32), np.full(n, 0xFFFFFFFF, np.uint32)


def chain_operands(first, a, b, r_or, r_xor, zero, one):
    """the operands of a chain by name: R is the first-level result of `first`, R' the other one"""
    return {"A": a, "B": b, "R": r_or if first == OR else r_xor, "R'": r_xor if first == OR else r_or, "0": zero, "1": one}


class Level:
    """a vector inside the model: words, kinds, block facts"""

    def __init__(self, words, kinds):
        self.w, self.k, self.f = words, np.asarray(kinds, np.int64), block_facts(words)


def model_op(op, compress, x, y):
    r = apply_op(op, x.w, y.w)
    fr = block_facts(r)
    return Level(r, model_kinds(op, compress, x.k, x.f, y.k, y.f, fr))


def model_chain():
    """-> {(first name, link name): Level} and the two first-level results, all under opt_none"""
    p = short_pair()
    a, b = [Level(p.words(s, True), import_kinds(p.words(s, True), True)) for s in (0, 1)]
    r_or, r_xor = model_op(OR, False, a, b), model_op(XOR, False, a, b)
    z, o = [Level(w, import_kinds(w, True)) for w in chain_constants()]
    out = {}
    for f in CHAIN_FIRST:
        v = chain_operands(f, a, b, r_or, r_xor, z, o)
        for name, op, x, y in CHAIN_LINKS:
            out[OP_NAMES[f], name] = model_op(op, False, v[x], v[y])
    return out, {"or": r_or, "xor": r_xor}


# ---------------------------------------------------------------------------------------------------------------------
# what the fixture holds (tests/golden/make_pair_golden.py, tests/test_pair_host.py)
# ---------------------------------------------------------------------------------------------------------------------
def fixture_pairs():
    """name -> (pair, flavours)"""
    out = {"short": (short_pair(), FLAVOURS), "long%d" % FIXTURE_N: (long_pair(FIXTURE_N), FLAVOURS),
           "cut": (cut_pair(), ((True, True), (False, False)))}
    return out


def _entry(v, nblocks):
    k = (v.flatten()[0].tolist() + [0] * nblocks)[:nblocks]
    return {"kinds": kinds_str(k), "count": v.count(), "sha": sha(v.to_words(nblocks * BW))}


def oracle_fixture(orc):
    """the whole fixture from an oracle (the reference writes it, the port reproduces it): import_words and op2 only"""
    out = {"pairs": {}, "chain": {}}
    for name, (p, fls) in fixture_pairs().items():
        per = {}
        for fl in fls:
            va, vb = [orc.import_words(p.words(s, fl[s]), fl[s], p.words(s, fl[s]).size * 32 - p.cut) for s in (0, 1)]
            e = {"operands": [kinds_str(v.flatten()[0]) for v in (va, vb)]}
            for op in OPS:
                for cm in (0, 1):
                    e["%s.%s" % (OP_NAMES[op], "compress" if cm else "none")] = _entry(orc.op2(op, va, vb, bool(cm)), p.nblocks)
            per[flavour_name(fl)] = e
        out["pairs"][name] = per
    p = short_pair()
    a, b = [orc.import_words(p.words(s, True), True, p.nbits) for s in (0, 1)]
    r_or, r_xor = orc.op2(OR, a, b, False), orc.op2(XOR, a, b, False)
    z, o = [orc.import_words(w, True, p.nbits) for w in chain_constants()]
    for f in CHAIN_FIRST:
        v = chain_operands(f, a, b, r_or, r_xor, z, o)
        for name, op, x, y in CHAIN_LINKS:
            out["chain"]["%s:%s" % (OP_NAMES[f], name)] = _entry(orc.op2(op, v[x], v[y], False), p.nblocks)
    return out


def model_entry(e, op, compress):
    r, _, cnt = e.result(op)
    nb = e.pair.nblocks
    return {"kinds": kinds_str(e.result_kinds(op, compress)), "count": cnt, "sha": sha(pad_blocks(r)[:nb * BW])}


# ---------------------------------------------------------------------------------------------------------------------
# tail cases: each its own small pair, results in closed form
# ---------------------------------------------------------------------------------------------------------------------
SLAB_SPARSE = ((16, (0, 1, 13, 14, 15, 16)), (2048, (1791, 1792, 2047, 2048)))      # live * 8 < nblocks * 7: 13 / 1,791 compact


def slab_sparse_words(nblocks):
    """a raw vector of nblocks bit-blocks (seeded 30 % words)"""
    return _pair(("sparse", nblocks), lambda: _raw_filler(4100 + nblocks, nblocks))


def slab_sparse_mask(nblocks, k):
    """the columns in which the mask is FULL: k of them, spread over the vector (the first and the last among them when k >= 2)"""
    if k == 0: return np.zeros(0, np.int64)
    return np.unique(np.round(np.linspace(0, nblocks - 1, k)).astype(np.int64)) if k > 1 else np.array([nblocks // 3], np.int64)


TRIM_N = 2048
TRIM_CASES = ("none_out", "three_out", "all_out")


def trim_pair(which):
    """laid-out path (operands with GAP blocks, opt_none, 2,048 blocks), one pair per branch of the GAP slab's trim:
    none_out    A = gA, B = gB in every column, AND: no GAP block comes out, the slab is given back
    three_out   the same but for three columns of (gA, gA): 3 GAP blocks out of operands whose GAP slabs hold 2,048: moved to a right-sized slab
    all_out     A = gA, B = gS, OR: every block a GAP block of gA's length, more than half of the operands' bound: the slab is kept"""
    cols = [("gA", "gS" if which == "all_out" else "gB")] * TRIM_N
    if which == "three_out":
        for c in (0, 1000, TRIM_N - 1): cols[c] = ("gA", "gA")
    return _pair(("trim", which), lambda: Pair("trim." + which, cols)), (OR if which == "all_out" else AND)


TAIL_NBLOCKS = 20481
TAIL_WG0 = 256 * 4                          # op2_loop = 1: 256 workgroups of 4 waves; workgroup 0 owns columns {0..3} + 1024 k


def tail_columns(n_cand):
    """the columns of workgroup 0, as many as candidates asked for: 80 = {0..3} + 1024 k for k < 20, 81 adds column 20 * 1024"""
    cols = [j + TAIL_WG0 * k for k in range(20) for j in range(4)]
    if n_cand == 81: cols.append(20 * TAIL_WG0)
    assert len(cols) == n_cand and max(cols) < TAIL_NBLOCKS
    return cols


TAIL_CLASSES = ("gA", "dfew")              # GAP x GAP of at most 703 runs: every result column of workgroup 0 is a GAP candidate


def tail_ranges(n_cand, side):
    """the [left, right] ranges of an operand that is NULL outside workgroup 0's columns and holds there, in every column, the
    1-runs of gA (side 0) / dfew (side 1): one GAP block per column, nothing dense on the host"""
    bits = _BITS[TAIL_CLASSES[side]]
    d = np.diff(np.concatenate([[0], bits.astype(np.int8), [0]]))
    lo, hi = np.flatnonzero(d == 1).astype(np.uint64), (np.flatnonzero(d == -1) - 1).astype(np.uint64)
    base = np.asarray(tail_columns(n_cand), np.uint64) * np.uint64(B)
    return np.stack([(base[:, None] + lo[None, :]).ravel(), (base[:, None] + hi[None, :]).ravel()], axis=1)


def tail_expect(n_cand, op):
    """(columns, words of one such column, count of the whole result) of A op B"""
    w = apply_op(op, WORDS[TAIL_CLASSES[0]], WORDS[TAIL_CLASSES[1]])
    return tail_columns(n_cand), w, popcount(w) * n_cand
