"""Inputs and expected values of the index-list pipeline tests (bmx_pipeline_run_indices): operand vectors whose block columns
cycle through the four block kinds, the arg-groups run over them, and the expected CSR from an oracle (the C port, or the
reference where it is built): agg_and_sub(and, sub).to_words() per group, the positions of its ones, restricted to the block
columns of the run."""
import numpy as np

B = 65536
NULL, FULL, BIT, GAP = 0, 1, 2, 3
NBITS = 6 * B + 321
NCOLS = 7


def _block(kind, rng, dense):
    """65,536 bits of the given kind as bytes of 0 / 1.  dense: a block that survives a long AND list (few zeros); else few ones."""
    if kind == NULL:
        return np.zeros(B, np.uint8)
    if kind == FULL:
        return np.ones(B, np.uint8)
    if kind == BIT:                                        # ~2,000 isolated bits of the minority value: > 1,280 runs, a bit-block
        b = (rng.random(B) < 0.03).astype(np.uint8)
        return (1 - b) if dense else b
    b = np.zeros(B, np.uint8)                              # GAP: ~40 runs of the minority value
    for s in rng.integers(0, B - 600, 40):
        b[s:s + int(rng.integers(1, 500))] = 1
    return (1 - b) if dense else b


def kinds_of(name, i, c):
    """the kind planned for block column c of operand `name`[i]"""
    if name == "a":                                        # AND material: FULL / BIT / GAP in turn, vectors 0..5 NULL in column i
        return NULL if (i < 6 and c == i) else (FULL, BIT, GAP)[(i + c) % 3]
    if name == "s":                                        # SUB material: NULL / BIT / GAP / NULL in turn, vectors 0..2 FULL in column i + 1
        return FULL if (i < 3 and c == i + 1) else (NULL, BIT, GAP, NULL)[(i + c) % 4]
    return GAP                                             # "g": GAP blocks only, long 1-runs; "h": GAP blocks only, short 1-runs


def operand_bits(name, i, nbits=NBITS):
    rng = np.random.default_rng(1000 * (ord(name[0]) - 96) + i)
    ncols = (nbits + B - 1) // B
    bits = np.concatenate([_block(kinds_of(name, i, c), rng, dense=(name not in "sh")) for c in range(ncols)])
    if name == "d":                                        # the disjoint pair: positions = i (mod 997)
        bits = (np.arange(bits.size) % 997 == i).astype(np.uint8)
    bits[nbits:] = 0
    return bits


def words_of(bits):
    return np.packbits(bits, bitorder="little").view(np.uint32)


OPERANDS = [("a", i) for i in range(24)] + [("s", i) for i in range(8)] + [("g", i) for i in range(4)] + [("d", 0), ("d", 1)]


def grid_groups():
    """the arg-groups of the kinds grid as (AND keys, SUB keys): AND lists of 1, 2, 3, 4, 5, 8, 9 and 17 operands (both sides of
    every batch of the operand fold), SUB lists of 0 to 5, and the special rows"""
    a = lambda *ix: [("a", i) for i in ix]
    s = lambda *ix: [("s", i) for i in ix]
    g = lambda *ix: [("g", i) for i in ix]
    long_ = list(range(6, 23))
    return [
        (a(6), []), (a(0), s(0)), (a(7, 8), s(1, 2)), (a(1, 9, 10), s(3)), (a(6, 7, 8, 9), s(0, 1, 2, 3, 4)),
        (a(10, 11, 12, 13, 14), s(5, 6, 7)), (a(*long_[:8]), s(4, 5)), (a(*long_[:9]), s(6)), (a(*long_), s(7, 3, 5, 6)),
        (a(*long_) , []),
        (a(6, 9, 12), []),                                 # all FULL in columns 0 and 3: ROW_FULL, 65,536 ids from one column
        (a(6, 9, 12), s(4)),                               # ... with a SUB list (ROW_ONES)
        (g(0, 1, 2), []), (g(0, 1), g(3)),                 # GAP-only AND groups
        ([], []), ([], s(1)),                              # empty AND lists: empty segments
        ([("d", 0), ("d", 1)], []),                        # a disjoint pair: zero hits
        (a(7, 7, 8, 7), s(2, 2)),                          # repeated operands
        (a(8, 13), a(13)),                                 # the same vector in AND and SUB: nothing
        (s(1, 2), []), (s(5), a(3)), (a(2, 3, 4, 5), []),  # sparse AND material; dense SUB material; NULLs in four columns
        (a(0, 1, 2, 3, 4, 5, 6), []),                      # a NULL in every whole column but the last
        (g(1) + a(11), s(0) + g(2)),                       # GAP and bit-block operands on both sides
    ]


def chunk_groups():
    """70 arg-groups over the same operands (chunk borders)"""
    rng = np.random.default_rng(77)
    base = grid_groups()
    out = []
    for k in range(70):
        if k % 7 == 3:
            out.append(base[k % len(base)])
            continue
        na, ns = int(rng.integers(1, 6)), int(rng.integers(0, 4))
        out.append(([("a", int(i)) for i in rng.integers(6, 24, na)], [("s", int(i)) for i in rng.integers(0, 8, ns)]))
    return out


def oracle_operands(orc, keys=OPERANDS, nbits=NBITS):
    return {k: orc.import_words(words_of(operand_bits(*k, nbits=nbits)), True, nbits) for k in keys}


def device_operands(bm, ctx, pv):
    """the oracle's block tables uploaded as they are: the device vectors hold exactly the kinds the oracle chose"""
    return {k: bm.bvector.from_block_table(ctx, v.nbits, *v.flatten()) for k, v in pv.items()}


def expected_csr(orc, pv, groups, nb_from=0, nb_to=None, ncols=NCOLS):
    """-> (offsets, ids): per group the ones of agg_and_sub(and, sub) inside block columns [nb_from, nb_to)"""
    nb_to = ncols if nb_to is None else min(nb_to, ncols)
    parts = []
    for an, su in groups:
        if not an:                                         # an empty AND list is skipped (src/bmaggregator.h:1352)
            parts.append(np.zeros(0, np.uint64))
            continue
        w = orc.agg_and_sub([pv[k] for k in an], [pv[k] for k in su]).to_words(ncols * 2048)
        ids = np.flatnonzero(np.unpackbits(np.ascontiguousarray(w, np.uint32).view(np.uint8), bitorder="little")).astype(np.uint64)
        parts.append(ids[(ids >= nb_from * B) & (ids < nb_to * B)])
    offsets = np.zeros(len(groups) + 1, np.uint64)
    offsets[1:] = np.cumsum([p.size for p in parts], dtype=np.uint64)
    return offsets, (np.concatenate(parts) if parts else np.zeros(0, np.uint64))


def make_pipeline(bm, ctx, gv, groups):
    pipe = bm.aggregator.pipeline(ctx, bm.agg_opt_disable_bvects_and_counts)
    for an, su in groups:
        ag = pipe.add()
        for k in an: ag.add(gv[k], 0)
        for k in su: ag.add(gv[k], 1)
    pipe.complete()
    return pipe
