"""Constructed cases for bm::rank_compressor on the device (k_rankc_* of bmx_kernels15.h, DESIGN_KERNELS.md 2.21): every border of
extract and deposit met exactly by a named case.  Shared by make_rankc_border_golden.py and the tests.

A case is one index vector and a list of source vectors; every source goes through both directions.  A vector (class V) is the
ascending positions of its ones after a prefix of FULL blocks (the prefix is 0 everywhere but in grid R, where 65,536 FULL blocks put
the ranks past 2^32) plus the storage kind of every block, because vectors are built by upload (bvector.from_block_table): GAP versus
bit-block is part of a case.  The answers are the closed forms of rankc_cases.py (model_compress / model_decompress on the part after
the prefix, the identity on the prefix) and table_of_positions.  plan() restates what the kernels decide per block -- window, source
kinds, shortcut, word form per 256-word row for deposit; feeders, signed offset, word form per row and the words split by an image
border for extract -- so that the host test can prove that a case meets the border it names.

The three constants (RANKC_NET_ROW, extract's `ca >= 1024u`, the automatic path's `inb * 2048ull`) are read from the sources when the
module is imported: a retune moves the cases with it (and the recorded reference subset then fails loudly).

Grids: W one word through both forms; D the deposit window; E the extract geometry; R ranks past 2^32 (each with a one-block twin)."""
from __future__ import annotations

import os
import re

import numpy as np

from import_cases import record, sha
from rankc_cases import model_compress, model_decompress, oracle_compress, oracle_decompress, oracle_vec, table_of_positions

NULL, FULL, BIT, GAP = 0, 1, 2, 3
B = 65536
BW = 2048
U = np.uint64
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
CSRC = os.path.join(ROOT, "bitmagic_amd", "csrc")
MAX_GAP_RUNS = 1275                 # what the cases store as a GAP block (the upload takes up to 1,279)


def read_constants() -> dict:
    """the three thresholds, from the text of the sources (nothing is compiled)"""
    k15 = open(os.path.join(CSRC, "bmx_kernels15.h")).read()
    hip = open(os.path.join(CSRC, "bmx.hip")).read()
    net = re.search(r"^#define\s+RANKC_NET_ROW\s+(\d+)u\b", k15, re.M)
    ext = re.search(r"const bool net = ca >= (\d+)u;", k15)
    auto = re.search(r"\(dir == 0 && total < \(uint64_t\)inb \* (\d+)ull\) \? 0 : 1;", hip)
    assert net and ext and auto, "rank compression thresholds not found in bmx_kernels15.h / bmx.hip"
    assert "const bool net = tot >= RANKC_NET_ROW;" in k15
    return {"RANKC_NET_ROW": int(net.group(1)), "EXT_NET_CA": int(ext.group(1)), "AUTO_PER_BLOCK": int(auto.group(1))}


CONSTANTS = read_constants()
NET_ROW, EXT_NET_CA, AUTO_PER_BLOCK = CONSTANTS["RANKC_NET_ROW"], CONSTANTS["EXT_NET_CA"], CONSTANTS["AUTO_PER_BLOCK"]


# ---- the word forms, transcribed (word_moves / word_extract_net / word_deposit_net), and the bit-by-bit rule -------------------
def _sh(i): return np.uint32(i)


def prefix_xor32(x):
    for s in (1, 2, 4, 8, 16):
        x = x ^ (x << _sh(s))
    return x


def word_moves(m):
    m = m.copy(); mk = ~m << _sh(1); mv = []
    for i in range(5):
        mp = prefix_xor32(mk); v = mp & m; mv.append(v)
        m = (m ^ v) | (v >> _sh(1 << i)); mk = mk & ~mp
    return mv


def word_extract_net(x, m):
    mv = word_moves(m); x = x & m
    for i in range(5):
        t = x & mv[i]; x = (x ^ t) | (t >> _sh(1 << i))
    return x


def word_deposit_net(x, m):
    mv = word_moves(m)
    for i in range(4, -1, -1):
        t = x << _sh(1 << i); x = (x & ~mv[i]) | (t & mv[i])
    return x & m


def word_extract_loop(x, m):
    """a step per bit position: r |= 1 << popc(m & ((1 << p) - 1)) for every one p of x & m"""
    r = np.zeros_like(m); x = x & m
    for p in range(32):
        below = m & np.uint32((1 << p) - 1)
        k = popcount32(below)
        r |= ((x >> _sh(p)) & np.uint32(1)) << k.astype(np.uint32)
    return r


def word_deposit_loop(x, m):
    r = np.zeros_like(m); k = np.zeros(m.shape, np.uint32)
    for p in range(32):
        mb = (m >> _sh(p)) & np.uint32(1)
        r |= (((x >> np.minimum(k, np.uint32(31))) & np.uint32(1)) & mb) << _sh(p)
        k += mb
    return r


def popcount32(w):
    w = np.ascontiguousarray(w, np.uint32)
    return np.unpackbits(w.view(np.uint8).reshape(-1, 4), axis=1).sum(axis=1).reshape(w.shape).astype(np.int64)


def bit_by_bit_extract(x: int, m: int) -> int:
    r = k = 0
    for p in range(32):
        if (m >> p) & 1:
            r |= ((x >> p) & 1) << k; k += 1
    return r


def bit_by_bit_deposit(x: int, m: int) -> int:
    r = k = 0
    for p in range(32):
        if (m >> p) & 1:
            r |= ((x >> k) & 1) << p; k += 1
    return r


def catalogue() -> np.ndarray:
    """the mask words of grid W: 263 words, 249 of them distinct (32 + 31 + 31 + 32 + 10 + 3 + 124: the families as listed, the zero
    word included; they overlap, 1 is a single bit and a low prefix)"""
    c = [1 << k for k in range(32)]
    c += [(1 << k) - 1 for k in range(1, 32)]
    c += [(0xFFFFFFFF << k) & 0xFFFFFFFF for k in range(1, 32)]
    c += [0xFFFFFFFF ^ (1 << k) for k in range(32)]
    for p in (0x55555555, 0x33333333, 0x0F0F0F0F, 0x00FF00FF, 0x0000FFFF):
        c += [p, p ^ 0xFFFFFFFF]
    c += [0x80000001, 0xFFFFFFFF, 0]
    rng = np.random.default_rng(1)
    for pc in range(1, 32):
        for _ in range(4):
            c.append(int(sum(1 << int(b) for b in rng.choice(32, pc, replace=False))))
    return np.array(c, np.uint32)


CATALOGUE = catalogue()
_CAT_PERM = np.random.default_rng(2).permutation(CATALOGUE.size)
_SLOTS = np.random.default_rng(3).permutation(256)


def cat_part(i: int, n: int) -> np.ndarray:
    """part i of the seeded split of the catalogue into n parts"""
    return CATALOGUE[_CAT_PERM[i::n]]


# ---- vectors ---------------------------------------------------------------------------------------------------------------
class V:
    """ones: ascending positions at or beyond prefix * 65,536; blocks [0, prefix) are FULL.  kinds: block -> BIT | GAP where the
    case fixes the storage; elsewhere a block of 65,536 ones is FULL, one of at most MAX_GAP_RUNS runs a GAP block, any other a
    bit-block"""

    def __init__(self, ones, nbits: int, kinds=None, prefix: int = 0):
        self.ones = np.ascontiguousarray(ones, U)
        assert self.ones.size < 2 or (np.diff(self.ones.astype(np.int64)) > 0).all()
        self.prefix = int(prefix)
        assert not self.ones.size or int(self.ones[0]) >= self.prefix * B
        self.nbits = int(nbits)
        assert self.nbits >= self.prefix * B and (not self.ones.size or int(self.ones[-1]) < self.nbits)
        self.forced = dict(kinds or {})
        self._off = self._tab = None

    @property
    def nblocks(self) -> int: return (self.nbits + B - 1) // B

    @property
    def count(self) -> int: return self.prefix * B + int(self.ones.size)

    def offsets(self) -> dict:
        """block -> the in-block offsets of its ones (blocks after the prefix that hold ones)"""
        if self._off is None:
            blk = (self.ones >> U(16)).astype(np.int64)
            ub, first = np.unique(blk, return_index=True)
            parts = np.split((self.ones & U(0xFFFF)).astype(np.int64), first[1:]) if ub.size else []
            self._off = {int(b): p for b, p in zip(ub, parts)}
        return self._off

    def block_counts(self) -> np.ndarray:
        bc = np.zeros(self.nblocks, np.int64)
        bc[:self.prefix] = B
        for b, o in self.offsets().items(): bc[b] = o.size
        return bc

    def table(self):
        """-> kinds, offs, bit_slab, gap_slab for bvector.from_block_table"""
        if self._tab is None:
            kinds = np.zeros(self.nblocks, np.uint8); offs = np.zeros(self.nblocks, np.uint32)
            kinds[:self.prefix] = FULL
            bit_parts, gap_parts, gpos = [], [], 0
            for b, off in sorted(self.offsets().items()):
                bits = np.zeros(B, np.uint8); bits[off] = 1
                ends = np.flatnonzero(np.diff(bits)).astype(np.uint16)
                runs = ends.size + 1
                want = self.forced.get(b)
                kind = want if want is not None else FULL if off.size == B else GAP if runs <= MAX_GAP_RUNS else BIT
                assert kind != GAP or runs <= MAX_GAP_RUNS, (b, runs)
                assert kind != FULL or off.size == B
                kinds[b] = kind
                if kind == GAP:
                    g = np.concatenate([[np.uint16((runs << 3) | int(bits[0]))], ends, [np.uint16(65535)]]).astype(np.uint16)
                    offs[b] = gpos; gap_parts.append(g); gpos += g.size
                elif kind == BIT:
                    offs[b] = len(bit_parts); bit_parts.append(np.packbits(bits, bitorder="little").view(np.uint32))
            self._tab = (kinds, offs, np.concatenate(bit_parts) if bit_parts else np.zeros(0, np.uint32),
                         np.concatenate(gap_parts) if gap_parts else np.zeros(0, np.uint16))
        return self._tab

    def block_kinds(self) -> np.ndarray: return self.table()[0]

    def explicit(self) -> np.ndarray:
        """all ones, the prefix included (twins and ordinary cases only)"""
        assert self.prefix <= 64
        return np.concatenate([np.arange(self.prefix * B, dtype=U), self.ones])


class Case:
    def __init__(self, name: str, idx: V, srcs, flavour: str = "avx2", twin: str | None = None, claims=None):
        self.name, self.grid, self.idx, self.srcs, self.flavour, self.twin = name, name.split("/")[0], idx, list(srcs), flavour, twin
        self.claims = dict(claims or {})
        assert len({n for n, _ in self.srcs}) == len(self.srcs)

    def __repr__(self): return "Case(%s)" % self.name

    def src(self, sname: str) -> V: return dict(self.srcs)[sname]

    def port_checked(self) -> bool: return self.idx.nblocks <= 64 and all(s.nblocks <= 64 for _, s in self.srcs)

    def as_dict(self, sname: str) -> dict:
        s = self.src(sname)
        return {"idx": self.idx.explicit(), "idx_nbits": self.idx.nbits, "src": s.ones, "src_nbits": s.nbits, "flavour": self.flavour}


# ---- the closed forms ------------------------------------------------------------------------------------------------------
def compress_positions(idx: V, src_ones: np.ndarray) -> np.ndarray:
    kb = U(idx.prefix * B)
    lo, hi = src_ones[src_ones < kb], src_ones[src_ones >= kb]
    return np.concatenate([lo, kb + model_compress(idx.ones, hi)]).astype(U)


def decompress_positions(idx: V, src_ones: np.ndarray) -> np.ndarray:
    kb = U(idx.prefix * B)
    s = src_ones[src_ones < U(idx.count)]
    lo, hi = s[s < kb], s[s >= kb]
    return np.concatenate([lo, model_decompress(idx.ones, hi - kb)]).astype(U)


def and_positions(idx: V, src_ones: np.ndarray) -> np.ndarray:
    kb = U(idx.prefix * B)
    return np.concatenate([src_ones[src_ones < kb], np.intersect1d(src_ones[src_ones >= kb], idx.ones, assume_unique=True)]).astype(U)


DIRECTIONS = ("compress", "decompress")
_EXPECTED = {}


def expected(case: Case, sname: str, direction: str) -> dict:
    """-> nbits_out, count, pos, ids_sha, opt0, opt1 (records of table_of_positions); computed once"""
    key = (case.name, sname, direction)
    if key not in _EXPECTED:
        s = case.src(sname)
        if direction == "compress":
            pos, nbits_out = compress_positions(case.idx, s.ones), case.idx.count
        else:
            pos, nbits_out = decompress_positions(case.idx, s.ones), case.idx.nbits
        _EXPECTED[key] = {"nbits_out": int(nbits_out), "count": int(pos.size), "pos": pos, "ids_sha": sha(pos.astype("<u8")),
                          "opt0": table_of_positions(pos, nbits_out, False), "opt1": table_of_positions(pos, nbits_out, True)}
    return _EXPECTED[key]


def expected_record(case: Case, sname: str, direction: str) -> dict:
    e = expected(case, sname, direction)
    return {k: e[k] for k in ("nbits_out", "count", "ids_sha", "opt0", "opt1")}


# ---- the same through an oracle (the C port or the reference) ----------------------------------------------------------------
def _oracle_result(o, pos: np.ndarray, nbits_out: int) -> dict:
    """set_bit per position on an empty vector of the oracle, flatten, optimize(), flatten again: what rankc_cases records"""
    t = o.new(nbits_out)
    for p in pos:
        t.set_bit(int(p))
    t.nbits = nbits_out
    cnt = t.count()
    opt0 = record(*t.flatten())
    t.optimize()
    t.nbits = nbits_out
    return {"nbits_out": int(nbits_out), "count": int(cnt), "opt0": opt0, "opt1": record(*t.flatten()),
            "ids_sha": sha(np.sort(pos).astype("<u8"))}


def _oracle_index(o, idx: V):
    if idx.nbits <= 64 * B:
        return oracle_vec(o, idx.explicit(), idx.nbits)
    v = o.new(idx.nbits)
    if idx.prefix: v.set_range(0, idx.prefix * B - 1)
    for p in idx.ones: v.set_bit(int(p))
    v.optimize()
    v.nbits = idx.nbits
    return v


def oracle_record(o, case: Case, sname: str, direction: str) -> dict:
    """rank / select of the oracle's own index, set_bit, optimize, flatten: rankc_cases.oracle_compress / oracle_decompress where
    the index fits their import (64 blocks), the same steps with the index built by set_range + set_bit beyond"""
    s = case.src(sname)
    if case.idx.nbits <= 64 * B and s.nbits <= 64 * B:
        d = case.as_dict(sname)
        r = oracle_compress(o, d) if direction == "compress" else oracle_decompress(o, d, s.ones)
    else:
        rs = o.rs_build(_oracle_index(o, case.idx))
        assert int(rs.count()) == case.idx.count
        if direction == "compress":
            a = and_positions(case.idx, s.ones)
            r = _oracle_result(o, rs.rank(a) - U(1) if a.size else np.zeros(0, U), case.idx.count)
        else:
            t = s.ones[s.ones < U(case.idx.count)]
            pos, found = rs.select(t + U(1)) if t.size else (np.zeros(0, U), np.ones(0, bool))
            assert found.all()
            r = _oracle_result(o, pos, case.idx.nbits)
    return r


# ---- what the kernels decide ---------------------------------------------------------------------------------------------------
def _rows(off: np.ndarray) -> np.ndarray: return np.bincount(off >> 13, minlength=8)


def _words(off: np.ndarray) -> np.ndarray: return np.bincount(off >> 5, minlength=BW)


_FULL_OFF = np.arange(B, dtype=np.int64)


def _idx_off(idx: V, b: int):
    return _FULL_OFF if b < idx.prefix else idx.offsets().get(b)


def plan(case: Case) -> dict:
    """per source: deposit[b] for every index block b the kernel computes a window for (from the last prefix block on), extract[t]
    for every target block t (from the last prefix block on)"""
    idx = case.idx
    inb, K = idx.nblocks, idx.prefix
    bc = idx.block_counts()
    P = np.cumsum(bc)
    total = int(P[-1]) if inb else 0
    ikinds = idx.block_kinds()
    nbt = (total + B - 1) // B
    first = max(K - 1, 0)
    out = {"inb": inb, "total": total, "nbt": nbt, "P": P, "auto_path": 0 if total < inb * AUTO_PER_BLOCK else 1, "deposit": {}, "extract": {}}
    wpop = {b: _words(_idx_off(idx, b)) for b in range(first, inb) if bc[b]}
    for sname, s in case.srcs:
        skinds, snb = s.block_kinds(), s.nblocks
        soff = s.offsets()
        dep = {}
        for b in range(first, inb):
            if ikinds[b] == NULL or not bc[b]: continue
            r0, r1 = int(P[b - 1]) if b else 0, int(P[b])
            sb0, sb1 = r0 >> 16, (r1 - 1) >> 16
            d0 = int(skinds[sb0]) if sb0 < snb else NULL
            d1 = int(skinds[sb1]) if sb1 != sb0 and sb1 < snb else NULL
            cut = "null" if d0 == NULL and d1 == NULL else "full" if d0 == FULL and (sb1 == sb0 or d1 == FULL) else None
            tot = _rows(_idx_off(idx, b))
            start = r0 & 0xFFFF
            o = start + np.cumsum(wpop[b]) - wpop[b]
            dep[b] = {"r0": r0, "r1": r1, "start": start, "len": r1 - r0, "sb0": sb0, "sb1": sb1, "d0": d0, "d1": d1,
                      "d0_in_range": sb0 < snb, "d1_in_range": sb1 < snb, "shortcut": cut, "idx_kind": int(ikinds[b]),
                      "tot": tot.tolist(), "form": ["net" if t >= NET_ROW else "loop" for t in tot],
                      "unaligned": bool(((o & 31) != 0)[wpop[b] > 0].any()), "last_lds_word": (start + r1 - r0 - 1) >> 5}
        out["deposit"][sname] = dep
        ext = {}
        for t in range(first, nbt):
            lo = t * B; hi = min(lo + B, total)
            b0 = int(np.searchsorted(P, lo, "right")); b1 = min(int(np.searchsorted(P, hi - 1, "right")), inb - 1)
            e = {"lo": lo, "hi": hi, "b0": b0, "b1": b1, "feeders": b1 - b0 + 1, "first_offset": (int(P[b0 - 1]) if b0 else 0) - lo,
                 "ties_lo": int((P == lo).sum()), "ties_hi": int((P == hi - 1).sum()), "blocks": {}, "lo_split": [], "hi_split": [],
                 "lo_word_border": [], "null_source_feeders": []}
            for b in range(b0, b1 + 1):
                sk = int(skinds[b]) if b < snb else NULL
                if ikinds[b] == NULL or not bc[b]: continue
                if sk == NULL: e["null_source_feeders"].append(b); continue
                ioff = _idx_off(idx, b)
                a = ioff if sk == FULL else np.intersect1d(ioff, soff.get(b, np.zeros(0, np.int64)), assume_unique=True)
                ca = _rows(a)
                base = (int(P[b - 1]) if b else 0) - lo
                o = base + np.cumsum(wpop[b]) - wpop[b]
                c = wpop[b]
                aw = _words(a)
                for w in np.flatnonzero((o < 0) & (o + c > 0) & (aw > 0)): e["lo_split"].append((b, int(w), int(-o[w])))
                for w in np.flatnonzero((o < B) & (o + c > B) & (aw > 0)): e["hi_split"].append((b, int(w), int(B - o[w])))
                for w in np.flatnonzero((o == 0) & (c > 0)): e["lo_word_border"].append((b, int(w)))
                e["blocks"][b] = {"offset": base, "src_kind": sk, "idx_kind": int(ikinds[b]), "ca": ca.tolist(),
                                  "form": ["net" if x >= EXT_NET_CA else "loop" if x else "none" for x in ca]}
            ext[t] = e
        out["extract"][sname] = ext
    return out


# ---- building blocks ------------------------------------------------------------------------------------------------------
def _scatter(count: int, seed: int, universe: int = B) -> np.ndarray:
    return np.sort(np.random.default_rng(seed).choice(universe, size=count, replace=False)).astype(np.int64)


def _parts(rng, n: int, k: int) -> np.ndarray:
    """n as k positive parts"""
    cuts = np.sort(rng.choice(n - 1, size=k - 1, replace=False)) + 1 if k > 1 else np.zeros(0, np.int64)
    return np.diff(np.concatenate([[0], cuts, [n]]))


def _runs(count: int, seed: int, k: int | None = None) -> np.ndarray:
    """count ones in at most 300 runs of ones: a block that fits a GAP block whatever its count"""
    if count == B: return _FULL_OFF
    zeros = B - count
    k = max(1, min(count, zeros - 1, 300 if k is None else k))
    rng = np.random.default_rng(seed)
    ones_len = _parts(rng, count, k)
    gaps = _parts(rng, zeros + 2, k + 1); gaps[0] -= 1; gaps[-1] -= 1
    start = np.cumsum(gaps[:-1]) + np.concatenate([[0], np.cumsum(ones_len[:-1])])
    return np.concatenate([np.arange(s, s + n) for s, n in zip(start, ones_len)]).astype(np.int64)


def _vec(blocks, nbits: int | None = None, prefix: int = 0) -> V:
    """blocks: per block after the prefix None (NULL) or (offsets, kind | None)"""
    ones, kinds = [], {}
    for i, blk in enumerate(blocks):
        if blk is None: continue
        off, kind = blk
        b = prefix + i
        if len(off): ones.append(U(b * B) + np.asarray(off, np.int64).astype(U))
        if kind is not None and len(off): kinds[b] = kind
    ones = np.concatenate(ones) if ones else np.zeros(0, U)
    return V(ones, (prefix + len(blocks)) * B if nbits is None else nbits, kinds, prefix)


def _by_count(counts, seed: int) -> V:
    """an index of the given ones per block: 65,536 FULL, else runs stored as a GAP block or scattered ones stored as a bit-block,
    in the pattern G B B G (so blocks two apart differ as well)"""
    blocks = []
    for i, c in enumerate(counts):
        if not c: blocks.append(None)
        elif c == B: blocks.append((_FULL_OFF, None))
        elif (i + i // 2) % 2 == 0: blocks.append((_runs(c, seed + i), GAP))
        else: blocks.append((_scatter(c, seed + i), BIT))
    return _vec(blocks)


def _subset(ones: np.ndarray, seed: int, p: float = 0.5) -> np.ndarray:
    return ones[np.random.default_rng(seed).random(ones.size) < p]


def _rank_rand(cnt: int, seed: int, p: float = 0.5) -> np.ndarray:
    return np.flatnonzero(np.random.default_rng(seed).random(cnt) < p).astype(U)


def _src(ones, nbits: int, kinds=None) -> V:
    return V(np.unique(np.asarray(ones, U)), nbits, kinds)


def _P(idx: V) -> np.ndarray: return np.cumsum(idx.block_counts())


def _standard_sources(idx: V, seed: int):
    """index space: the index's content under another handle, a random half of it, the first one of every block"""
    firsts = np.array([b * B + int(o[0]) for b, o in sorted(idx.offsets().items())], U)
    return [("twin", V(idx.ones.copy(), idx.nbits, idx.forced)), ("half", _src(_subset(idx.ones, seed), idx.nbits)), ("firsts", _src(firsts, idx.nbits))]


# ---- grid W -------------------------------------------------------------------------------------------------------------------
def _row_words(content) -> np.ndarray:
    assert len(content) <= 256, len(content)
    row = np.zeros(256, np.uint32)
    row[_SLOTS[:len(content)]] = np.array(content, np.uint32)
    return row


def _offsets_of_words(words: np.ndarray) -> np.ndarray:
    return np.flatnonzero(np.unpackbits(np.ascontiguousarray(words, np.uint32).view(np.uint8), bitorder="little")).astype(np.int64)


def w_deposit_rows():
    """-> the 8 rows of the W index block: row 2q holds quarter q of the catalogue padded to RANKC_NET_ROW - 1 ones (the loop),
    row 2q + 1 the same quarter padded to RANKC_NET_ROW (the network).  A quarter leaves 190 free slots, so single-bit fillers alone
    cannot reach the threshold: a row takes the fewest all-ones fillers (the m == ~0 shortcut, neither form) that let single-bit
    fillers make the total exact"""
    rows = []
    for q in range(4):
        part = [int(w) for w in cat_part(q, 4)]
        ones = int(popcount32(np.array(part, np.uint32)).sum())
        free = 256 - len(part)
        for target in (NET_ROW - 1, NET_ROW):
            need = target - ones
            assert need >= 0, "a quarter of the catalogue no longer fits under the loop threshold"
            k = 0 if target == NET_ROW - 1 else need // 32
            while (need - 32 * k) + k > free: k += 1
            singles = need - 32 * k
            assert 0 <= singles and singles + k <= free
            rows.append(_row_words(part + [0xFFFFFFFF] * k + [1 << ((7 * i) % 32) for i in range(singles)]))
    return rows


EXT_VARIANTS = ("self", "lowest", "highest", "random")


def select_bits(m: np.ndarray, variant: str, seed: int) -> np.ndarray:
    m = np.asarray(m, np.uint32)
    if variant == "self": return m.copy()
    if variant == "lowest": return m & (~m + np.uint32(1))
    if variant == "highest":
        return np.array([(1 << (int(x).bit_length() - 1)) if x else 0 for x in m], np.uint32)
    return m & np.random.default_rng(seed).integers(0, 1 << 32, m.size, dtype=np.uint64).astype(np.uint32)


W_EXT_FILLERS = 32


def w_extract_rows():
    """-> (index rows, {variant: source rows}): 16 rows; row 2e + side holds eighth e of the catalogue and 32 all-ones fillers;
    the source words under the masks are the variant's choice, the source words under the fillers make ca exactly
    EXT_NET_CA - 1 (side 0, the loop) or EXT_NET_CA (side 1, the network)"""
    irows, srows = [], {v: [] for v in EXT_VARIANTS}
    for e in range(8):
        part = cat_part(e, 8)
        for side, target in enumerate((EXT_NET_CA - 1, EXT_NET_CA)):
            irows.append(_row_words([int(w) for w in part] + [0xFFFFFFFF] * W_EXT_FILLERS))
            for v in EXT_VARIANTS:
                sel = select_bits(part, v, 100 + e)
                need = target - int(popcount32(sel).sum())
                assert 0 <= need <= 32 * W_EXT_FILLERS, "an eighth of the catalogue no longer fits under the extract threshold"
                fill = [0xFFFFFFFF] * (need // 32) + ([(1 << (need % 32)) - 1] if need % 32 else [])
                fill += [0] * (W_EXT_FILLERS - len(fill))
                srows[v].append(_row_words([int(w) for w in sel] + fill))
    return irows, srows


def _grid_w():
    rows = w_deposit_rows()
    idx = _vec([(_offsets_of_words(np.concatenate(rows)), BIT)])
    cnt = idx.count
    hole = np.delete(np.arange(cnt, dtype=U), cnt // 2)
    srcs = [("random_half", _src(_rank_rand(cnt, 41), cnt, {0: BIT})), ("alternating", _src(np.arange(0, cnt, 2, dtype=U), cnt)),
            ("ones_but_one", _src(hole, cnt))]
    yield Case("W/deposit", idx, srcs, claims={"rows": 8})
    irows, srows = w_extract_rows()
    iw = np.concatenate(irows)
    idx = _vec([(_offsets_of_words(iw[:BW]), BIT), (_offsets_of_words(iw[BW:]), BIT)])
    srcs = []
    for v in EXT_VARIANTS:
        sw = np.concatenate(srows[v])
        srcs.append((v, _vec([(_offsets_of_words(sw[:BW]), BIT), (_offsets_of_words(sw[BW:]), BIT)])))
    yield Case("W/extract", idx, srcs, claims={"rows": 16})


# ---- grid D -------------------------------------------------------------------------------------------------------------------
D_STARTS = (0, 1, 31, 32, 33, 65504, 65535)
D_LENS_SMALL, D_LENS_BIG = (1, 2, 32, 33), (65535, 65536)


def _chain(lens):
    """the ones per index block such that every (start, length) of D_STARTS x lens is the window of one block; fillers move the
    running count to the next start"""
    counts, want, r = [], [], 0
    for ln in lens:
        for s in D_STARTS:
            f = (s - r) % B
            if f: counts.append(f); r += f
            want.append((len(counts), s, ln))
            counts.append(ln); r += ln
    return counts, want


def _window_sources(idx: V, seed: int):
    """rank space: a random half, the first bit of every window, the last bit of every window"""
    P = _P(idx); cnt = idx.count
    bc = idx.block_counts()
    r0 = (P - bc)[bc > 0]; r1 = P[bc > 0]
    return [("random_half", _src(_rank_rand(cnt, seed), cnt)), ("window_firsts", _src(r0, cnt)), ("window_lasts", _src(r1 - 1, cnt))]


# source kinds along the rank space of D/kinds: every ordered pair of {NULL, FULL, GAP, bit} is a pair of neighbours
D_KIND_SEQ = (NULL, NULL, FULL, NULL, GAP, NULL, BIT, FULL, FULL, GAP, FULL, BIT, GAP, GAP, BIT, BIT, NULL)
D_KINDS_START, D_KINDS_LEN = 65000, 1000


def _grid_d():
    for name, lens in (("D/chain_small", D_LENS_SMALL), ("D/chain_big", D_LENS_BIG)):
        counts, want = _chain(lens)
        idx = _by_count(counts, 1000 if lens is D_LENS_SMALL else 2000)
        yield Case(name, idx, _window_sources(idx, 7), claims={"windows": want})
    idx = _by_count([B, B], 2500)                                              # every window one source block, o & 31 == 0 throughout
    yield Case("D/aligned_full", idx, _window_sources(idx, 7), claims={"windows": [(0, 0, B), (1, 0, B)]})
    # every pair of source kinds under a straddling window; the three shortcuts and their near misses; the source's end
    counts = [D_KINDS_START]
    for _ in range(16): counts += [D_KINDS_LEN, B - D_KINDS_LEN]
    idx = _by_count(counts, 3000)
    cnt = idx.count
    blocks = []
    for j, k in enumerate(D_KIND_SEQ):
        blocks.append(None if k == NULL else (_FULL_OFF, None) if k == FULL else (_runs(30000, 3100 + j, 200), GAP) if k == GAP
                      else (_scatter(32768, 3100 + j), BIT))
    last = cnt - 16 * B                                                        # the 17th block is partial (and NULL)
    assert 0 < last <= B and D_KIND_SEQ[16] == NULL
    kinds_src = _vec(blocks, cnt)
    P = _P(idx)
    wa, wb = 9, 12                                                             # a straddling window and one inside a block
    ra, rb = (int(P[wa - 1]), int(P[wa])), (int(P[wb - 1]), int(P[wb]))
    on = np.concatenate([np.arange(*ra, dtype=U), np.arange(*rb, dtype=U)])
    touched = sorted({ra[0] >> 16, (ra[1] - 1) >> 16, rb[0] >> 16, (rb[1] - 1) >> 16})
    around = np.concatenate([np.arange(b * B, (b + 1) * B, dtype=U) for b in touched])
    off = np.setdiff1d(around, on)
    bitk = {b: BIT for b in touched}
    half = _rank_rand(cnt, 17)
    srcs = [("kinds", kinds_src), ("ones_on_the_window", _src(on, cnt, bitk)), ("zero_on_the_window", _src(off, cnt, bitk)),
            ("ends_at_sb1", _src(half[half < U(5 * B)], 5 * B)), ("ends_at_sb0", _src(half[half < U(4 * B)], 4 * B)),
            ("bits_around_count", _src(np.concatenate([_rank_rand(cnt, 18, 0.01), [cnt - 1, cnt, cnt + 1, cnt + B + 5]]), cnt + 3 * B))]
    yield Case("D/kinds", idx, srcs, claims={"straddling": [1 + 2 * j for j in range(16)], "near_miss": (wa, wb), "source_end": wa})


# ---- grid E -------------------------------------------------------------------------------------------------------------------
E_FEEDERS = (1, 2, 3, 4, 5, 8, 9)
# (word, in-word rank) of the target border inside the split index block; rank 0: the border is the word's low end
E_SPLITS = ((40, 1), (300, 16), (1000, 31), (7, 0), (4, 0), (256, 0))
E_TIE_COUNTS = (40000, 25536, 30000, 35536, 0, B, 0, 0, 0, 20000, 45536, 5000, 60536, B - 1, 0, 0, 100)
E_TOTALS = {1: (0, 1), 65535: (32768, 32767), 65536: (32768, 32768), 65537: (32768, 32768, 1), 131072: (B, 30000, 35536)}


def _split_block(w0: int, seed: int):
    """words [0, w0 + 8) hold 16 ones each, word w0 all 32: the ones before word w0 are 16 * w0"""
    rng = np.random.default_rng(seed)
    words = np.zeros(BW, np.uint32)
    for w in range(w0 + 8):
        words[w] = sum(1 << int(b) for b in rng.choice(32, 16, replace=False))
    words[w0] = 0xFFFFFFFF
    return words


def _grid_e():
    counts = []
    for n in E_FEEDERS:
        counts += [B // n + B % n] + [B // n] * (n - 1)
    idx = _by_count(counts, 4000)
    yield Case("E/feeders", idx, _standard_sources(idx, 8), claims={"feeders": E_FEEDERS})

    blocks, r, split_at = [], 0, []
    for j, (w0, k) in enumerate(E_SPLITS, 1):
        words = _split_block(w0, 4100 + j)
        r0 = j * B - 16 * w0 - k
        f = r0 - r
        assert 0 < f < B
        blocks.append((_runs(f, 4200 + j), GAP))
        split_at.append((len(blocks), w0, k))
        off = _offsets_of_words(words)
        blocks.append((off, BIT)); r = r0 + off.size
    blocks.append((_scatter(100, 4300), BIT))
    idx = _vec(blocks)
    only = np.concatenate([U(b * B) + np.arange(32 * w0, 32 * w0 + 32, dtype=U) for b, w0, _ in split_at])
    srcs = _standard_sources(idx, 9)[:2] + [("split_words_only", _src(only, idx.nbits))]
    yield Case("E/split", idx, srcs, claims={"split_at": split_at})

    idx = _by_count(E_TIE_COUNTS, 4400)
    no11 = idx.ones[(idx.ones >> U(16)) != U(11)]
    srcs = [("twin_without_block_11", _src(no11, idx.nbits)), ("half_without_block_11", _src(_subset(no11, 10), idx.nbits)),
            ("short", _src(_subset(idx.ones[idx.ones < U(2 * B + 5)], 11), 2 * B + 5)), _standard_sources(idx, 12)[2]]
    yield Case("E/ties", idx, srcs, claims={"null_source_block": 11})

    for total, cs in E_TOTALS.items():
        idx = _by_count(cs, 4500 + len(cs))
        yield Case("E/total_%d" % total, idx, _standard_sources(idx, 13)[:2], claims={"total": total})

    idx = _vec([(_scatter(3, 4600 + b), BIT if b % 2 else GAP) for b in range(8)])
    mids = np.array([b * B + int(o[1]) for b, o in sorted(idx.offsets().items())], U)
    yield Case("E/shared_word", idx, _standard_sources(idx, 14)[:1] + [("mids", _src(mids, idx.nbits))], claims={"blocks": 8})

    idx = _vec([(_runs(20000, 4700), GAP), (_scatter(20000, 4701), BIT), (_scatter(3000, 4702), BIT)])
    full = _vec([(_FULL_OFF, None), (_FULL_OFF, None), None])
    yield Case("E/full_source", idx, [("full", full), ("full_short", _vec([(_FULL_OFF, None)]))], claims={})

    for side in (0, 1):                                                        # the automatic path's line, both sides
        total = 4 * AUTO_PER_BLOCK - 1 + side
        idx = _by_count([total - 3 * (total // 4)] + [total // 4] * 3, 4800)
        yield Case("E/auto_%s" % ("below", "at")[side], idx, _standard_sources(idx, 15)[:2], claims={"total": total, "path": side})


# ---- grid R -------------------------------------------------------------------------------------------------------------------
R_PREFIX = 65536


def _r_case(K: int) -> Case:
    kb = K * B
    idx = _vec([(_scatter(20000, 5000), BIT), (_runs(30000, 5001), GAP), (_FULL_OFF, None), (_scatter(500, 5002, B - 100), BIT)],
               (K + 4) * B - 77, K)
    cnt, tail = idx.count, idx.ones
    nt = tail.size
    zeros = np.setdiff1d(U(kb) + _scatter(300, 5003).astype(U), tail)          # positions of the first tail block outside idx
    pre = np.unique(np.concatenate([[0, 5, B - 1, kb - B, kb - 2], np.random.default_rng(5004).integers(0, kb, 200)])).astype(U)
    sparse_c = np.concatenate([pre, [kb - 1], tail[:2], _subset(tail[2:], 5005, 0.02), zeros])
    full_c = np.concatenate([np.arange(kb - B, kb, dtype=U), _subset(tail, 5006, 0.01)])
    sparse_d = np.concatenate([pre, [kb - 1, kb, kb + 1], U(kb) + _scatter(3000, 5007, nt).astype(U), [cnt - 1]])
    blocks_d = np.concatenate([U(kb - B) + _scatter(300, 5008).astype(U), [kb - 1, kb], U(kb) + _scatter(300, 5009).astype(U)])
    srcs = [("sparse_index_space", _src(sparse_c, idx.nbits)), ("full_block_before_the_tail", _src(full_c, idx.nbits)),
            ("sparse_rank_space", _src(sparse_d, cnt)), ("blocks_around_the_prefix_end", _src(blocks_d, cnt))]
    big = K == R_PREFIX
    return Case("R/past_2_32" if big else "R/twin", idx, srcs, "avx2_64" if big else "avx2", "R/twin" if big else None, {"prefix": K})


def _grid_r():
    yield _r_case(R_PREFIX)
    yield _r_case(1)


def _all():
    out = {}
    for g in (_grid_w, _grid_d, _grid_e, _grid_r):
        for c in g():
            assert c.name not in out
            out[c.name] = c
    return out


_CASES = None


def cases() -> dict:
    global _CASES
    if _CASES is None: _CASES = _all()
    return _CASES


N_CASES = {"W": 2, "D": 4, "E": 12, "R": 2}

# what goes to the reference: all of W; the D and E cases that name a shortcut, a tie or a split word; one R case, sparse source
RECORDED = (("W/deposit", None), ("W/extract", None), ("D/kinds", None), ("E/split", None), ("E/ties", None),
            ("R/past_2_32", ("sparse_index_space",)))


def recorded():
    """-> (case, source name) pairs of the reference subset"""
    cs = cases()
    return [(cs[n], s) for n, only in RECORDED for s, _ in cs[n].srcs if only is None or s in only]
