"""Constructed cases for the AND / AND-SUB fold (tests/test_and_fold_host.py, tests/test_gpu_and_fold.py): operands built
from explicit run lists so that every decision point of the fold is met on purpose, each with its answer in closed form.

A case is a list of AND operands and a list of SUB operands over three block columns.  Block 1 carries the case; block 0
(every AND operand a dense GAP block sharing one long 1-run: the column survives with a known count) and block 2 (every
vector holds one bit of its own: the column dies at the second AND operand) catch state left over between items.  Operands of
the bit-block kind carry the same decoys as bit-blocks (isolated bits on top), so that a bit-only case stays bit-only.

Block 1 is made of layers that live in disjoint regions:
  [0, 16384)        C: the shared part of exactly P bits, in every AND operand (clustered: one run; spread: runs of 4 bits at
                    a stride of 48 + a remainder run, a GAP block for every P up to 1025; `edge`: bits 0 and 65535 belong to C)
  [16400, 19900)    L: a second shared layer of 2,000 bits (250 runs of 8), carried by the first e AND operands only
  [20000, 21000)    own parts of GAP operands: three isolated bits in the operand's residue class mod 320 (pairwise disjoint)
  [24000, 60000)    own parts of bit-block operands, even positions: ~8,900 isolated bits, the two classes mod 4 in turn (so two
                    neighbours of a list share nothing but C); odd positions: the killers and SUB operands of the bit kind
  [60500, 62300)    killers of the GAP kind: an AND operand without any bit of C, L or an own part
  [63000, 65000)    the SUB operands' own bits (GAP kind)
After two AND operands the accumulator is exactly C (+ L while every operand so far carries it).

The constants below restate the kernels' thresholds; the grids are laid around them (DESIGN_KERNELS.md 2.2, 2.12).
No GPU, no oracle: pure NumPy."""
import numpy as np

B = 65536
BW = 2048
NBLOCKS = 3
NBITS = NBLOCKS * B
NULL, FULL, BIT, GAP = 0, 1, 2, 3

SPARSE_CAP = 1024                      # bmx_device.h: sparse state at pop <= SPARSE_CAP
NJ_BUCKETS = (1, 2, 3, 4, 6, 8, 12, 16)   # gap_apply_sparse: sparse_test<NJ> dispatch, nj = (alive + 63) >> 6
HEAD, HEAD_FROM, LANE_STEP = 8, 32, 64    # gap_apply_list: head of 8 operands when n >= 32, then 64 operands per lane step
PIPE_U = 4                             # pipe_chain: accumulator tested once per 2 U operands
PIECE_CHUNKS, CHUNK_WORDS = 64, 8      # ar_union_list: a piece is 64 chunks of 8 words (header + run ends)
MAX_GAP_LEN = 1275                     # longest run list bit_import keeps as a GAP block (the host test finds it by importing)

N_AND = (1, 2, 3, 4, 5, 7, 8, 9, 12, 13, 15, 16, 17, 31, 32, 33, 39, 40, 41, 71, 72, 73, 74, 136, 137, 255, 256, 257)
N_SUB = (0, 1, 2, 8, 9)
N_AND_WITH_SUB = (1, 8, 33, 73)
P_GRID = (1, 2, 63, 64, 65, 128, 129, 192, 193, 256, 257, 384, 385, 512, 513, 768, 769, 1023, 1024, 1025)

RUN0 = (1000, 50000)                   # block 0: the 1-run every AND operand shares
L_RUNS = [(16400 + 14 * k, 16400 + 14 * k + 7) for k in range(250)]


# ---------------------------------------------------------------------------------------------------------------------
# blocks
# ---------------------------------------------------------------------------------------------------------------------
def block_of(runs=(), bits=()):
    """65,536 booleans: the 1-runs [s, e] (inclusive) and the single positions"""
    b = np.zeros(B, bool)
    for s, e in runs:
        assert 0 <= s <= e < B
        b[s:e + 1] = True
    if len(bits):
        b[np.asarray(bits, np.int64)] = True
    return b


def block_of_ends(ends, sbit):
    """the block whose run k (1-based) ends at ends[k - 1] (ends[-1] == 65535) and whose first run has value sbit"""
    ends = np.asarray(ends, np.int64)
    assert ends[-1] == B - 1 and (np.diff(ends) > 0).all() and ends[0] >= 0
    v = np.zeros(B, np.int8)
    v[ends[:-1] + 1] = 1                                    # a run starts behind every end but the last
    return ((np.cumsum(v) + sbit) & 1).astype(bool)


def gap_level(ln):
    return 0 if ln <= 124 else 1 if ln <= 252 else 2 if ln <= 508 else 3


def gap_words(b):
    """the GAP form of a block: [len << 3 | level << 1 | start bit, end of run 1, ..., 65535]"""
    ends = np.concatenate([np.flatnonzero(b[1:] != b[:-1]), [B - 1]])
    ln = ends.size
    return np.concatenate([[(ln << 3) | (gap_level(ln) << 1) | int(b[0])], ends]).astype(np.uint16)


def len_sbit(b):
    return int(np.count_nonzero(b[1:] != b[:-1])) + 1, int(b[0])


def words_of(bits):
    return np.packbits(bits, bitorder="little").view(np.uint32).copy()


def kind_of(b):
    """the kind bit_import (optimize) gives the block: one run -> NULL / FULL, up to MAX_GAP_LEN runs -> GAP"""
    ln, s = len_sbit(b)
    return (FULL if s else NULL) if ln == 1 else GAP if ln <= MAX_GAP_LEN else BIT


class Operand:
    """one vector of three blocks.  words: its bits; kinds: the intended kind per block; table: the vector is uploaded from its
    block table (all blocks GAP, as constructed -- a GAP block of one run is not something an import produces)"""
    _next = [0]

    def __init__(self, role, b1, table=False, note="", kind="gap", index=0):
        self.uid = uid = Operand._next[0]
        Operand._next[0] += 1
        assert uid < 8000
        self.role, self.table, self.note = role, table, note
        own2 = 3 + 8 * uid
        if kind == "gap":
            # AND: the shared long run + one bit of its own; SUB operands stay clear of the run.  Block 2: one bit of its own
            b0 = block_of([RUN0], [50100 + uid]) if role == "and" else block_of((), [60000 + uid % 5000])
            b2 = block_of((), [own2])
        else:
            # the same as bit-blocks: isolated bits on top, the two classes mod 4 by the operand's list index (neighbours of a list share
            # none of them); SUB operands on the odd positions
            k = np.arange(3000)
            dense = 52000 + 4 * k + (2 * (index & 1) if role == "and" else 1)
            b0 = block_of([RUN0] if role == "and" else (), dense)
            b2 = block_of((), np.concatenate([dense - 30000, [own2]]))
        blocks = (b0, b1, b2)
        self.words = words_of(np.concatenate(blocks))
        self.kinds = tuple(GAP if table else kind_of(b) for b in blocks)
        self.len1, self.sbit1 = len_sbit(b1)
        self.gaps = [gap_words(b) if k == GAP else None for b, k in zip(blocks, self.kinds)]

    def block(self, n):
        return np.unpackbits(self.words[n * BW:(n + 1) * BW].view(np.uint8), bitorder="little").astype(bool)

    def block1(self):
        return self.block(1)

    def block_table(self):
        """kinds, offs, bit_slab, gap_slab of the flattened vector (table operands only)"""
        assert self.table
        offs = np.cumsum([0] + [g.size for g in self.gaps[:-1]]).astype(np.uint32)
        return np.full(NBLOCKS, GAP, np.uint8), offs, np.zeros(0, np.uint32), np.concatenate(self.gaps)


class Case:
    def __init__(self, grid, name, ands, subs, expect1, kind, **params):
        self.grid, self.name, self.ands, self.subs, self.kind = grid, name, list(ands), list(subs), kind
        p = dict(n_and=len(self.ands), n_sub=len(self.subs), d=None, P=None, e=None, len=None, sbit=None)
        p.update(params)
        self.params = p
        # closed form of the three blocks: block 0 keeps the shared run (+ the own bit of a lone AND operand), block 2 dies at the
        # second AND operand (a lone operand keeps its bit); SUB operands hold nothing there
        first = self.ands[0]
        lone = len(set(o.uid for o in self.ands)) == 1
        b0 = first.block(0) if lone else block_of([RUN0])
        b2 = first.block(2) if lone else np.zeros(B, bool)
        self.expect1 = expect1
        self.expect_words = words_of(np.concatenate([b0, expect1, b2]))
        self.expect_count = int(b0.sum()) + int(expect1.sum()) + int(b2.sum())
        self.under_test = None                              # G1: the operand whose len / start bit the case is about

    def __repr__(self):
        return "%s/%s %s" % (self.grid, self.name, " ".join("%s=%s" % kv for kv in self.params.items()))

    def first(self):
        """(found, position) of the first set bit"""
        nz = np.flatnonzero(self.expect_words)
        if not nz.size:
            return False, 0
        w = int(self.expect_words[nz[0]])
        return True, int(nz[0]) * 32 + ((w & -w).bit_length() - 1)

    def indices(self):
        return np.flatnonzero(np.unpackbits(self.expect_words.view(np.uint8), bitorder="little")).astype(np.uint64)


# ---------------------------------------------------------------------------------------------------------------------
# layers of block 1
# ---------------------------------------------------------------------------------------------------------------------
def shared_part(P, shape, edge):
    """C: exactly P positions"""
    pos = []
    if edge:
        pos = [B - 1] if P == 1 else [0, B - 1]
    n = P - len(pos)
    if shape == "clustered":
        pos += list(range(200, 200 + n))
    else:
        q, r = divmod(n, 4)
        for k in range(q):
            pos += list(range(200 + 48 * k, 200 + 48 * k + 4))
        pos += list(range(200 + 48 * q, 200 + 48 * q + r))
    pos = np.array(sorted(pos), np.int64)
    assert pos.size == P and np.unique(pos).size == P and (pos[(pos > 0) & (pos < B - 1)] < 16384).all()
    return pos


def _own_gap(i):
    return [20000 + (i % 320) + 320 * k for k in range(3)]


def _own_bit(i):
    k = np.arange(8999)
    return (24000 + 4 * k + 2 * (i & 1))[k % 251 != i % 251]


class Family:
    """the operands built on one shared part C: AND operands i = 0, 1, ... of either kind (with or without the layer L),
    killers, SUB operands.  Built once, selected from by the cases."""

    def __init__(self, P, shape="clustered", edge=False):
        self.P, self.shape, self.edge = P, shape, edge
        self.C = shared_part(P, shape, edge)
        self.cache = {}

    def _get(self, key, make):
        if key not in self.cache:
            self.cache[key] = make()
        return self.cache[key]

    def c_block(self, with_l=False):
        return block_of(L_RUNS if with_l else (), self.C)

    def and_op(self, i, kind="gap", with_l=False):
        def make():
            b = self.c_block(with_l)
            b[_own_gap(i) if kind == "gap" else _own_bit(i)] = True
            return Operand("and", b, note="and%d" % i, kind=kind, index=i)
        return self._get(("and", i, kind, with_l), make)

    def killer(self, i, kind="gap"):
        def make():
            if kind == "gap":
                b = block_of((), [60500 + 3 * (i % 300) + 900 * k for k in range(2)])
            else:
                b = block_of((), 24001 + 4 * np.arange(8999)[np.arange(8999) % 241 != i % 241])
            return Operand("and", b, note="killer%d" % i, kind=kind, index=i)
        return self._get(("kill", i, kind), make)

    def sub_op(self, tag, hit_runs=(), hit_bits=(), kind="gap"):
        """a SUB operand that removes the given runs / positions (of C, or of unused space) and otherwise holds bits of its own"""
        def make():
            b = block_of(hit_runs, hit_bits)
            n = len([k for k in self.cache if k[0] == "sub"])
            if kind == "gap":
                b[[63000 + 5 * (n % 390), 63001 + 5 * (n % 390) + 2]] = True
            else:
                b[24003 + 4 * np.arange(8999)[np.arange(8999) % 239 != n % 239]] = True
            return Operand("sub", b, note="sub:%s" % (tag,), kind=kind)
        return self._get(("sub", tag, kind), make)

    def sub_all(self, kind="gap"):
        """removes every bit of C (and of L)"""
        return self.sub_op("all", [(1, 19990)], [0, B - 1] if self.edge else (), kind)

    def pool_subs(self, n, kind="gap"):
        """the fixed SUB operands: 0 -- its 1-run ENDS exactly on a bit of C (the bit goes, its upper neighbour in a clustered C
        survives); 1 -- its 1-run BEGINS exactly one past a bit of C (that bit survives); the others remove two bits each"""
        c = self.C[(self.C > 0) & (self.C < B - 1)]
        out = []
        for k in range(n):
            if not c.size:
                out.append(self.sub_op(("pool", k), kind=kind))
                continue
            if k == 0:
                e = int(c[min(10, c.size - 1)])
                runs = [(max(e - 2, 1), e)]
            elif k == 1:
                s = int(c[min(20, c.size - 1)]) + 1
                runs = [(s, s + 2)]
            else:
                s = int(c[min(30 + 7 * k, c.size - 1)])
                runs = [(s, s + 1)]
            out.append(self.sub_op(("pool", k), runs, kind=kind))
        return out

    def expect(self, ands_with_l, subs):
        b = self.c_block(ands_with_l)
        for s in subs:
            b &= ~s.block1()
        return b


def fold_case(grid, name, fam, n_and, kind="gap", subs=(), d=None, e=0, **params):
    """AND operands 0 .. n_and - 1 of the family (the first e with the layer L, a killer at index d) and the SUB operands"""
    ands = [fam.and_op(i, kind, with_l=(i < e)) for i in range(n_and)]
    if d is not None:
        ands[d] = fam.killer(d, kind)
    if n_and == 1:
        exp = ands[0].block1()
        for s in subs:
            exp &= ~s.block1()
    elif d is not None:
        exp = np.zeros(B, bool)
    else:
        exp = fam.expect(e >= n_and, subs)
    return Case(grid, name, ands, subs, exp, kind, d=d, P=fam.P, e=e if e else None, **params)


# ---------------------------------------------------------------------------------------------------------------------
# G1: run geometry of one GAP operand
# ---------------------------------------------------------------------------------------------------------------------
def g1_lens():
    """len in every residue mod 8 at one, two and three pieces of 512 words (header + len run ends)"""
    piece = PIECE_CHUNKS * CHUNK_WORDS
    out = list(range(1, 25)) + list(range(piece - 12, piece + 13)) + list(range(2 * piece - 12, 2 * piece + 13))
    return out + list(range(MAX_GAP_LEN - 7, MAX_GAP_LEN + 1))


def block_with_len(ln, sbit):
    """ln runs, the first of value sbit: run ends at a stride of 50 (+ a wobble, so that runs start and end at every position of a word)"""
    k = np.arange(1, ln)
    ends = np.concatenate([30 + 50 * k + (k * 7) % 13, [B - 1]])
    return block_of_ends(ends, sbit)


def g1_geometry_blocks():
    """1-runs whose first / last bit sits at positions 0, 1, 31 of a word, lengths 1 .. 65 and 3,000: same word, adjacent words
    (the difference-array pair that nets to nothing), long interiors; a run from bit 0 and a run up to bit 65535"""
    out = []
    for ln in (1, 2, 31, 32, 33, 63, 64, 65, 3000):
        runs = []
        for j, m in enumerate((0, 1, 31)):
            s = 4096 + 8192 * j + m                        # first bit at m mod 32
            runs.append((s, s + ln - 1))
            e = 4096 + 8192 * (j + 3) + 4064 + m           # last bit at m mod 32
            runs.append((e - ln + 1, e))
        out.append(("runs%d" % ln, block_of(runs)))
        out.append(("ends%d" % ln, block_of([(0, ln - 1), (B - ln, B - 1)])))
    return out + [(n + "inv", ~b) for n, b in out]


def _table_op(role, b1, note):
    return Operand(role, b1, table=True, note=note)


def grid_g1():
    cases = []
    ones = _table_op("and", np.ones(B, bool), "ones")       # the all-ones single-run GAP block
    full = Operand("and", np.ones(B, bool), note="full")    # imported: a FULL block (dropped from the AND list)
    assert full.kinds[1] == FULL and ones.kinds[1] == GAP and ones.len1 == 1

    def both_roles(name, b):
        ln, sb = len_sbit(b)
        xa, xs = _table_op("and", b, name), _table_op("sub", b, name)
        c = Case("G1", name + "/and", [xa, ones], [], b.copy(), "gap", len=ln, sbit=sb)
        c.under_test = xa
        cases.append(c)
        c = Case("G1", name + "/sub", [full], [xs], ~b, "gap", len=ln, sbit=sb)
        c.under_test = xs
        cases.append(c)

    for ln in g1_lens():
        for sb in (0, 1):
            both_roles("len%d.%d" % (ln, sb), block_with_len(ln, sb))
    for name, b in g1_geometry_blocks():
        both_roles(name, b)
    # alignment in a wave's chunk stream.  k_agg_and_rows deals the GAP operands of a list to its NW = wg / 64 waves as operand
    # w, w + NW, ... in list order (k_pipe_sort keeps that order from the back of the row), and a wave reads its operands as one
    # stream of 16-byte chunks.  A list of NW copies of the filler F followed by NW copies of the operand X therefore gives EVERY
    # wave the stream F, X: X starts at chunk nch(F) of the stream -- position 1 or 63 of the first piece, or 0 of the second
    # (at position 63 only X's header chunk lies in the first piece; its next run takes the dword before from the carry).  The
    # reversed list (the second group of the pipeline) puts X in front.  One list per workgroup size; under the other sizes
    # the same lists give other alignments.  F holds ones below bit 32768 and its runs above, X the other way round, so
    # F & X = X's lower half + F's upper half; in the SUB role the complements are subtracted from a FULL operand: same answer.
    for pos, flen in ((1, 7), (63, 503), (0, 511)):
        assert (flen + 8) >> 3 == (pos if pos else 64)
        for fs in (0, 1):
            for xs_ in (0, 1):
                k = np.arange(1, flen - (1 - fs))
                f = block_of_ends(np.concatenate([[0] if not fs else [], 32768 + 40 * k + (k * 5) % 11, [B - 1]]).astype(np.int64), fs)
                k = np.arange(1, 21)
                x = block_of_ends(np.concatenate([17 + 900 * k + (k * 3) % 32, [B - 1]]), xs_)
                x[32768:] = True
                assert len_sbit(f) == (flen, fs) and len_sbit(x)[1] == xs_ and len_sbit(x)[0] >= 16
                for nw in (2, 4, 8):
                    name = "align%d.f%d.x%d.nw%d" % (pos, fs, xs_, nw)
                    ln, sb = len_sbit(x)
                    fa, xa = _table_op("and", f, "filler"), _table_op("and", x, "x")
                    c = Case("G1", name + "/and", [fa] * nw + [xa] * nw, [], f & x, "gap", len=ln, sbit=sb)
                    c.under_test = xa
                    cases.append(c)
                    fsub, xsub = _table_op("sub", ~f, "filler"), _table_op("sub", ~x, "x")
                    c = Case("G1", name + "/sub", [full], [fsub] * nw + [xsub] * nw, f & x, "gap", len=ln, sbit=1 - sb)
                    c.under_test = xsub
                    cases.append(c)
    return cases


# ---------------------------------------------------------------------------------------------------------------------
# G2 .. G5
# ---------------------------------------------------------------------------------------------------------------------
_FAMILIES = {}


def family(P, shape="clustered", edge=False):
    key = (P, shape, edge)
    if key not in _FAMILIES:
        _FAMILIES[key] = Family(P, shape, edge)
    return _FAMILIES[key]


def grid_g2():
    """operand counts: every n_and without SUB operands, every n_sub at four n_and; both operand kinds over one pool"""
    fam = family(300)
    cases = []
    for kind in ("gap", "bit"):
        for n in N_AND:
            cases.append(fold_case("G2", "%s.n%d" % (kind, n), fam, n, kind))
        for n in N_AND_WITH_SUB:
            for ns in N_SUB[1:]:
                cases.append(fold_case("G2", "%s.n%d.s%d" % (kind, n, ns), fam, n, kind, subs=fam.pool_subs(ns, kind)))
    return cases


def death_indices(n):
    d = {0, 1, n - 1}
    for m in range(0, n + 1, 4):
        d |= {m - 1, m, m + 1}
    return sorted(x for x in d if 0 <= x < n)


def grid_g3():
    """where the accumulator dies: a killer at chosen indices of the AND list, death at the first SUB operand, death at the last
    SUB operand only.  GAP operands (P = 300: the list is in the sparse state from its second operand on; with the layer L on
    every operand it never is, and the head / lane steps find the empty accumulator), then bit-block operands, those also
    with n_and = 1 .. 17 (every residue of the 2 U stride of pipe_chain and its re-loaded tail)."""
    fam = family(300)
    cases = []
    for kind in ("gap", "bit"):
        ns_ = sorted(set(N_AND) | (set(range(1, 18)) if kind == "bit" else set()))
        for n in ns_:
            for d in death_indices(n):
                cases.append(fold_case("G3", "%s.n%d.d%d" % (kind, n, d), fam, n, kind, d=d))
        for n in N_AND_WITH_SUB:
            for ns in N_SUB[1:]:
                pool = fam.pool_subs(ns - 1, kind)
                cases.append(fold_case("G3", "%s.n%d.s%d.first" % (kind, n, ns), fam, n, kind, subs=[fam.sub_all(kind)] + pool, d_sub=0))
                cases.append(fold_case("G3", "%s.n%d.s%d.last" % (kind, n, ns), fam, n, kind, subs=pool + [fam.sub_all(kind)], d_sub=ns - 1))
    for n in (12, 33, 73, 137):                             # never sparse: the layer L on every operand
        for d in death_indices(n):
            cases.append(fold_case("G3", "gapdense.n%d.d%d" % (n, d), fam, n, "gap", d=d, e=n))
    return cases


def bucket_targets(P, plus):
    """survivor counts that take alive down one nj bucket at a time: 64 nj (+ plus) for the buckets below P's"""
    return [64 * nj + plus for nj in reversed(NJ_BUCKETS) if 64 * nj + plus < P] + [1]


def step_subs(fam, tag, targets):
    """SUB operands that leave targets[0], targets[1], ... survivors of C, spread evenly over C"""
    c = np.sort(fam.C)
    alive = np.ones(c.size, bool)
    out = []
    for k, t in enumerate(targets):
        if t >= alive.sum():
            continue
        keep = np.zeros(c.size, bool)
        live = np.flatnonzero(alive)
        keep[live[np.unique(np.round(np.linspace(0, live.size - 1, t)).astype(np.int64))]] = True
        assert keep.sum() == t
        out.append(fam.sub_op((tag, k), (), c[alive & ~keep]))
        alive = keep
    return out


def grid_g4():
    """how many survive: P on either side of every bucket of the sparse state and of SPARSE_CAP, both shapes (n_and 12: the head
    alone; 40: head + one lane step), the edge variants at n_and 12; then SUB lists that take the survivors down to 64 in one
    step and one bucket at a time (to 64 nj exactly and to 64 nj + 1)"""
    cases = []
    for shape in ("clustered", "spread"):
        for P in P_GRID:
            for edge, ns_ in ((False, (12, 40)), (True, (12,))):
                fam = family(P, shape, edge)
                lists = [("none", [])]
                if P > 1:
                    lists.append(("one", step_subs(fam, "one", [min(64, P - 1), min(63, P - 1) - (P <= 64)])))
                    lists.append(("steps", step_subs(fam, "steps", bucket_targets(P, 0))))
                    lists.append(("steps1", step_subs(fam, "steps1", bucket_targets(P, 1))))
                for n in ns_:
                    for tag, subs in lists:
                        if tag != "none" and len(subs) == 0: continue
                        cases.append(fold_case("G4", "%s%s.P%d.n%d.%s" % (shape, ".edge" if edge else "", P, n, tag), fam, n, "gap", subs=subs))
    return cases


def grid_g5():
    """where the sparse state is entered: the layer L on the first e operands (population P + 2000 up to operand e - 1, P from
    operand e on) in a short list and in one with a head and two lane steps; entry at list start -- bit-block operands that leave
    P bits before two or more GAP operands, SUB lists of 1 and 2 operands after a GAP AND list that left P bits"""
    fam = family(300)
    cases = []
    for n, es in ((12, (1, 2, 7, 8, 10, 11)), (137, (8, 9, 72, 73, 135))):
        for e in es:
            cases.append(fold_case("G5", "L.n%d.e%d" % (n, e), fam, n, "gap", e=e))
            cases.append(fold_case("G5", "L.n%d.e%d.s2" % (n, e), fam, n, "gap", e=e, subs=fam.pool_subs(2)))
    for P in (300, SPARSE_CAP, SPARSE_CAP + 1):
        f = family(P, "spread")
        for nbit in (1, 2, 9):
            for ngap in (2, 3):
                ands = [f.and_op(i, "bit") for i in range(nbit)] + [f.and_op(100 + i, "gap") for i in range(ngap)]
                cases.append(Case("G5", "mixed.P%d.b%d.g%d" % (P, nbit, ngap), ands, [], f.expect(False, []), "mixed", P=P))
                subs = f.pool_subs(2)
                cases.append(Case("G5", "mixed.P%d.b%d.g%d.s2" % (P, nbit, ngap), ands, subs, f.expect(False, subs), "mixed", P=P))
        for ns in (1, 2):
            cases.append(fold_case("G5", "sublist.P%d.s%d" % (P, ns), f, 5, "gap", subs=f.pool_subs(ns)))
    return cases


_GRIDS = {"G1": grid_g1, "G2": grid_g2, "G3": grid_g3, "G4": grid_g4, "G5": grid_g5}
_CACHE = {}
CHUNK = {"G1": 80, "G2": 16, "G3": 160, "G4": 60, "G5": 24}     # cases per parametrised test


def port_vec(orc, op, cache):
    """the operand inside an oracle: imported from its words, or -- table operands, in the port -- taken over as the GAP blocks it
    was built as (the reference imports them: a one-run GAP block becomes NULL / FULL there, the same bits)"""
    key = (orc.is_ref, op.uid)
    if key not in cache:
        if op.table and not orc.is_ref:
            cache[key] = orc.from_table(NBITS, *op.block_table())
        else:
            cache[key] = orc.import_words(op.words, True, NBITS)
    return cache[key]


def device_vec(bm, ctx, orc, op, cache, pcache):
    """the port's block table uploaded as it is: the device vector holds exactly the kinds the port chose"""
    if op.uid not in cache:
        cache[op.uid] = bm.bvector.from_block_table(ctx, NBITS, *port_vec(orc, op, pcache).flatten())
    return cache[op.uid]


N_CASES = {"G1": 472, "G2": 88, "G3": 2795, "G4": 462, "G5": 64}          # cases per grid (checked when a grid is built)


def grid(name):
    if name not in _CACHE:
        _CACHE[name] = _GRIDS[name]()
        assert len(_CACHE[name]) == N_CASES[name], (name, len(_CACHE[name]))
    return _CACHE[name]


def chunks():
    """(grid, chunk index) of every parametrised test, without building a grid"""
    return [(g, k) for g in _GRIDS for k in range((N_CASES[g] + CHUNK[g] - 1) // CHUNK[g])]


def chunk(name, k):
    return grid(name)[k * CHUNK[name]:(k + 1) * CHUNK[name]]
