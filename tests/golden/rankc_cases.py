"""The operands of rankc_ref.json (bm::rank_compressor, src/bmalgo.h:452-707) and the two ways the tests restate the
reference's per-bit rule.  Shared by make_rankc_golden.py and the tests; every operand comes from fixed seeds and is held as the
ascending positions of its ones.  The canonical form of a block table is import_cases.record().

  compress    for every one p of src & idx: bit count_to(p) - 1 of an empty vector of count(idx) bits (the body of
              compress_by_source's visitor, :673-674)
  decompress  for every one s of src below count(idx): bit select(s + 1) of an empty vector of idx's size (what decompress
              reaches through find_rank, :593-612)
then flatten (every touched block a bit-block), optimize(), flatten again."""
from __future__ import annotations

import zlib

import numpy as np

from import_cases import _alternating, record, sha  # noqa: F401

B = 65536
U = np.uint64


def _rand(seed: int, block: int, p: float) -> np.ndarray:
    return (block * B + np.flatnonzero(np.random.default_rng(seed).random(B) < p)).astype(U)


def _full(block: int) -> np.ndarray:
    return block * B + np.arange(B, dtype=U)


def _runs(block: int, seed: int, nruns: int) -> np.ndarray:
    """nruns long runs of ones: a GAP block that is not sparse"""
    cut = np.sort(np.random.default_rng(seed).choice(np.arange(1, B), size=2 * nruns, replace=False))
    return np.concatenate([block * B + np.arange(cut[2 * i], cut[2 * i + 1], dtype=U) for i in range(nruns)])


def _cat(*parts) -> np.ndarray:
    return np.unique(np.concatenate([np.asarray(p, U) for p in parts])) if parts else np.zeros(0, U)


def _subset(ids: np.ndarray, seed: int, p: float) -> np.ndarray:
    return ids[np.random.default_rng(seed).random(ids.size) < p]


def _case(idx, idx_nbits, src, src_nbits, flavour="avx2"):
    idx = np.asarray(idx, U); src = np.asarray(src, U)
    return {"idx": idx, "idx_nbits": int(max(idx_nbits, int(idx.max()) + 1 if idx.size else 0)),
            "src": src, "src_nbits": int(max(src_nbits, int(src.max()) + 1 if src.size else 0)), "flavour": flavour}


def cases():
    c = {}
    i30 = _cat(*[_rand(100 + b, b, 0.3) for b in range(3)])
    c["empty_src"] = _case(i30, 3 * B, np.zeros(0, U), 3 * B)
    c["empty_idx"] = _case(np.zeros(0, U), 2 * B + 5, _cat(_rand(1, 0, 0.2), _rand(2, 1, 0.01)), 2 * B + 5)
    c["src_equals_idx"] = _case(i30, 3 * B, i30.copy(), 3 * B)
    c["idx_full"] = _case(_cat(_full(0), _full(1), _full(2)), 3 * B, _cat(_rand(3, 0, 0.1), _rand(4, 1, 0.001), _runs(2, 5, 40)), 3 * B)
    c["idx_null_between"] = _case(_cat(_rand(6, 0, 0.3), _rand(7, 3, 0.3), _rand(8, 7, 0.3)), 9 * B,
                                  _cat(*[_rand(10 + b, b, 0.2) for b in range(9)]), 9 * B)
    ig = _cat(*[_rand(30 + b, b, 0.001) for b in range(16)])
    c["idx_gap"] = _case(ig, 16 * B, _cat(_subset(ig, 9, 0.5), _rand(50, 3, 0.05)), 16 * B)
    ib = _cat(*[_rand(60 + b, b, 0.3) for b in range(6)])
    c["idx_bit"] = _case(ib, 6 * B, _cat(*[_rand(70 + b, b, 0.1) for b in range(6)]), 6 * B)
    c["idx_mixed_src_every_kind"] = _case(
        _cat(_full(0), _rand(80, 1, 0.002), _rand(81, 2, 0.3), _full(4), _runs(5, 82, 60)), 6 * B,
        _cat(_rand(83, 0, 0.5), _full(1), _rand(84, 2, 0.003), _rand(85, 3, 0.4), _full(5)), 6 * B)
    isp = _cat(*[_rand(120 + b, b, 0.046) for b in range(24)])                       # ~3,000 ones per block: ~21 blocks per target block
    c["sparse_index_many_to_one"] = _case(isp, 24 * B, _subset(isp, 11, 0.5), 24 * B)
    idn = _cat(np.sort(np.random.default_rng(12).choice(B, size=40000, replace=False)).astype(U), _full(1), _full(2), _rand(13, 3, 0.9))
    c["dense_unaligned_prefix"] = _case(idn, 4 * B, _cat(_subset(idn[:40000], 14, 0.3), _full(1), _full(2), _rand(15, 3, 0.5)), 4 * B)
    c["src_shorter"] = _case(ib, 6 * B, _cat(_rand(16, 0, 0.4), _rand(17, 1, 0.4)[:-50]), 2 * B - 100)
    i2 = _cat(_rand(18, 0, 0.3), _rand(19, 1, 0.3))
    c["src_longer"] = _case(i2, 2 * B, _cat(*[_rand(20 + b, b, 0.3) for b in range(8)]), 8 * B)
    il = _cat(_rand(140, 0, 0.3), _rand(141, 2, 0.01), [3 * B + 76])
    c["last_bit_of_idx"] = _case(il, 3 * B + 77, _cat(_subset(il, 21, 0.5), [3 * B + 76]), 3 * B + 77)
    even = np.arange(0, 4 * B, 2, dtype=U)                                          # rank r <-> position 2r: 2 target blocks
    c["runs_1275"] = _case(even, 4 * B, 2 * _alternating(1, 1, 637), 4 * B)
    c["runs_1276"] = _case(even, 4 * B, 2 * _alternating(1, 0, 638), 4 * B)
    hi = 1 << 32
    i64 = _cat(_rand(150, 0, 0.005), _rand(151, 2, 0.005), hi - B + _rand(152, 0, 0.005), hi + _rand(153, 0, 0.01),
               hi + 3 * B + _rand(154, 0, 0.005), [hi + 4 * B - 1])
    c["beyond_2_32"] = _case(i64, hi + 4 * B, _cat(_subset(i64, 22, 0.5), [5, hi + 9]), hi + 4 * B, "avx2_64")
    return c


def decompress_sources(name: str, case: dict) -> dict:
    """the decompress inputs of a case -> name -> (ids, nbits): the compress output (the round trip must give back src & idx)
    and an independent random subset of [0, count(idx))"""
    cnt = int(case["idx"].size)
    comp = model_compress(case["idx"], case["src"])
    seed = zlib.crc32(name.encode())
    rnd = np.flatnonzero(np.random.default_rng(seed).random(cnt) < 0.3).astype(U)
    return {"roundtrip": (comp, cnt), "random": (rnd, cnt)}


# ---- the cumulative-sum model: positions in, positions out -----------------------------------------------------------------
def model_compress(idx: np.ndarray, src: np.ndarray) -> np.ndarray:
    a = np.intersect1d(src, idx, assume_unique=True)
    return np.searchsorted(idx, a).astype(U)                   # ones of idx before p = rank(p) - 1


def model_decompress(idx: np.ndarray, src: np.ndarray) -> np.ndarray:
    return idx[src[src < idx.size].astype(np.int64)].astype(U)


# ---- the same through an oracle (the C port or the reference): rank / select of its own index, set_bit, optimize, flatten -----
def words_of(ids: np.ndarray, nbits: int) -> np.ndarray:
    nblocks = (nbits + B - 1) // B
    bits = np.zeros(nblocks * B, np.uint8)
    bits[ids.astype(np.int64)] = 1
    return np.packbits(bits, bitorder="little").view(np.uint32)


def oracle_vec(o, ids: np.ndarray, nbits: int):
    """the vector of the given ones in the oracle, optimised (FULL / GAP / bit-blocks by content)"""
    if nbits <= 64 * B:
        return o.import_words(words_of(ids, nbits), True, nbits)
    v = o.new(nbits)
    for p in ids:
        v.set_bit(int(p))
    v.optimize()
    v.nbits = nbits
    return v


def ones_of(v) -> np.ndarray:
    w = v.to_words()
    nz = np.flatnonzero(w)
    bits = np.unpackbits(w[nz].view(np.uint8).reshape(-1, 4), axis=1, bitorder="little")
    wi, bi = np.nonzero(bits)
    return (nz[wi].astype(U) * 32 + bi.astype(U))


def _result(o, pos: np.ndarray, nbits_out: int) -> dict:
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


def oracle_compress(o, case: dict) -> dict:
    idx_v = oracle_vec(o, case["idx"], case["idx_nbits"])
    rs = o.rs_build(idx_v)
    if case["idx_nbits"] <= 64 * B:                            # the ones of src & idx from the oracle's own AND
        a = ones_of(o.op2(0, oracle_vec(o, case["src"], case["src_nbits"]), idx_v))
    else:
        a = np.intersect1d(case["src"], case["idx"], assume_unique=True)
    pos = rs.rank(a) - U(1) if a.size else np.zeros(0, U)      # count_to(p) - 1
    return _result(o, pos, int(rs.count()))


def oracle_decompress(o, case: dict, src: np.ndarray) -> dict:
    idx_v = oracle_vec(o, case["idx"], case["idx_nbits"])
    rs = o.rs_build(idx_v)
    s = src[src < U(rs.count())]
    if s.size:
        pos, found = rs.select(s + U(1))
        assert found.all()
    else:
        pos = np.zeros(0, U)
    return _result(o, pos, case["idx_nbits"])


def oracle_case(o, name: str, case: dict) -> dict:
    out = {"flavour": case["flavour"], "idx_count": int(case["idx"].size), "idx_nbits": case["idx_nbits"],
           "src_count": int(case["src"].size), "compress": oracle_compress(o, case)}
    for k, (ids, _) in decompress_sources(name, case).items():
        out["decompress_" + k] = oracle_decompress(o, case, ids)
    return out


def model_case(name: str, case: dict) -> dict:
    """nbits_out, count and the hash of the positions from the cumulative-sum model alone"""
    comp = model_compress(case["idx"], case["src"])
    out = {"compress": {"nbits_out": int(case["idx"].size), "count": int(comp.size), "ids_sha": sha(comp.astype("<u8"))}}
    for k, (ids, _) in decompress_sources(name, case).items():
        d = model_decompress(case["idx"], ids)
        out["decompress_" + k] = {"nbits_out": case["idx_nbits"], "count": int(d.size), "ids_sha": sha(np.sort(d).astype("<u8"))}
    return out


def table_of_positions(pos: np.ndarray, nbits_out: int, optimize: bool) -> dict:
    """record() of the table the rule gives for a set of positions, without any oracle: touched blocks are bit-blocks; with
    optimize one run of ones is FULL, fewer than 1,276 runs a GAP block (blocks_manager::optimize_bit_block,
    src/bmblocks.h:1412-1436)"""
    nblocks = (nbits_out + B - 1) // B
    kinds = np.zeros(nblocks, np.uint8); offs = np.zeros(nblocks, np.uint32)
    bit_parts, gap_parts, gpos = [], [], 0
    blk = (pos >> U(16)).astype(np.int64)
    for b in np.unique(blk):
        off = (pos[blk == b] & U(0xFFFF)).astype(np.int64)
        bits = np.zeros(B, np.uint8); bits[off] = 1
        ends = np.flatnonzero(np.diff(bits)).astype(np.uint16)            # run k ends at ends[k]
        runs = ends.size + 1
        if optimize and runs == 1:
            kinds[b] = 1
        elif optimize and runs < 1276:
            kinds[b] = 3; offs[b] = gpos
            g = np.concatenate([[np.uint16((runs << 3) | int(bits[0]))], ends, [np.uint16(65535)]]).astype(np.uint16)
            gap_parts.append(g); gpos += g.size
        else:
            kinds[b] = 2; offs[b] = len(bit_parts)
            bit_parts.append(np.packbits(bits, bitorder="little").view(np.uint32))
    return record(kinds, offs, np.concatenate(bit_parts) if bit_parts else np.zeros(0, np.uint32),
                  np.concatenate(gap_parts) if gap_parts else np.zeros(0, np.uint16))
