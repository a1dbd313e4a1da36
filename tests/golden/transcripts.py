#!/usr/bin/env python3
"""Transcripts of the oracle's differentials against the reference (tests/test_oracle_golden.py).

One function runs one fixed sequence of calls on either back-end of oracle/ (the C port or the reference built into
oracle/_ref) and returns what each call answered, as (label, value) pairs; arrays enter as short SHA-256 digests.
transcripts_ref.json holds the reference's transcripts, so the port is checked against the reference on machines
where oracle/_ref is not built.  Regenerate it where it is:

    python tests/golden/transcripts.py          # writes tests/golden/transcripts_ref.json
"""
from __future__ import annotations

import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "transcripts_ref.json")
SOAK_SEEDS = 80


def _d(a) -> str:
    a = np.ascontiguousarray(a)
    return hashlib.sha256(a.dtype.str.encode() + str(a.shape).encode() + a.tobytes()).hexdigest()[:16]


def vs_reference(O, port):
    """import kinds, pairwise ops and counts, AND-SUB / OR, shift-right-and, pipelines with and without a search limit,
    over five densities; inputs from the port's generator"""
    out = []
    rng = np.random.default_rng(7)
    nbits = 5 * 65536 + 77
    for dq in (40, 655, 6554, 40000, 65500):
        ws = []
        for v in range(5):
            w = port.gen_words(99, v, dq, nbits)
            for nb in range(6):
                r = rng.integers(0, 8)
                if r == 0: w[nb * 2048:(nb + 1) * 2048] = 0
                if r == 1: w[nb * 2048:(nb + 1) * 2048] = 0xFFFFFFFF
            ws.append(w)
        vs = [O.import_words(w) for w in ws]
        for i, p in enumerate(vs):
            out += [(f"{dq} import {i} kinds", _d(p.flatten()[0])), (f"{dq} import {i} count", p.count())]
        for op in range(4):
            out += [(f"{dq} op2 {op}", _d(O.op2(op, vs[0], vs[1]).to_words())), (f"{dq} count_op2 {op}", O.count_op2(op, vs[2], vs[3]))]
        out += [(f"{dq} agg_and_sub", _d(O.agg_and_sub(vs[:3], vs[3:]).to_words())), (f"{dq} agg_or", _d(O.agg_or(vs).to_words()))]
        for sel in ([0, 1], [4, 3, 2, 1, 0], [2, 2, 2], [0, 1, 2] * 15, [1] * 70):
            for opt, any_ in ((False, False), (True, False), (False, True)):
                t, f = O.agg_shift_right_and([vs[i] for i in sel], opt, any_)
                out += [(f"{dq} shift {sel[:5]} {opt} {any_}", [bool(f), _d(t.to_words()), _d(t.flatten()[0])])]
            out += [(f"{dq} shift count {sel[:5]}", int(O.agg_shift_right_and_count([vs[i] for i in sel])))]
        out += [(f"{dq} pipeline", [int(x) for x in O.pipeline_counts([(vs[:4], vs[4:]), (vs[1:], [])])])]
        for lim in (1, 7, 300, 70000, 0xFFFFFFFF):
            g = [(vs[:2], []), (vs[:1], vs[3:]), (vs[1:3], vs[:1]), (vs[4:], [])]
            out += [(f"{dq} pipeline limit {lim}", [int(x) for x in O.pipeline_counts_limit(g, lim)])]
    return out


KINDS = ["null", "full", "sparse", "mid", "dense", "runs", "half"]


def _block(rng, kind):
    w = np.zeros(2048, np.uint32)
    if kind == "full": w[:] = 0xFFFFFFFF
    elif kind == "sparse":
        pos = rng.choice(65536, size=int(rng.integers(1, 400)), replace=False); np.bitwise_or.at(w, pos >> 5, (np.uint32(1) << (pos & 31).astype(np.uint32)))
    elif kind == "mid": w[:] = rng.integers(0, 1 << 32, 2048, dtype=np.uint64).astype(np.uint32)
    elif kind == "dense":
        w[:] = 0xFFFFFFFF; pos = rng.choice(65536, size=int(rng.integers(1, 300)), replace=False); np.bitwise_and.at(w, pos >> 5, ~(np.uint32(1) << (pos & 31).astype(np.uint32)))
    elif kind == "runs":
        a = 0
        while a < 2048:
            l = int(rng.integers(1, 200)); w[a:a + l] = 0xFFFFFFFF if rng.integers(0, 2) else 0; a += l
    elif kind == "half": w[:1024] = 0xFFFFFFFF
    return w


def _last_nonempty(w):
    nzb = np.flatnonzero(w.reshape(-1, 2048).any(axis=1))
    return int(nzb[-1]) if nzb.size else -1


def soak_seed(O, seed):
    """one seed of tools/cpu_soak_oracle_vs_reference.py's randomized differential (random block tables incl.
    un-optimised and aliased operands; pairwise ops, aggregator in both opt modes, pipelines with OR target,
    find_first, shift-right-and, rank / select / count_range), the same draws in the same order"""
    out = []
    rng = np.random.default_rng(90000 + seed)
    nblk = int(rng.integers(1, 6)); nv = int(rng.integers(2, 7))
    ws = [np.concatenate([_block(rng, KINDS[int(rng.integers(0, len(KINDS)))]) for _ in range(nblk)]) for _ in range(nv)]
    opt = bool(rng.integers(0, 2))
    vs = [O.import_words(w, opt, nblk * 65536) for w in ws]
    out += [("import", [[_d(v.flatten()[0]), v.count()] for v in vs])]
    for op in range(4):
        i, j = (int(x) for x in rng.integers(0, nv, 2)); oc = bool(rng.integers(0, 2))
        a = O.op2(op, vs[i], vs[j], oc)
        out += [(f"op2 {op}", [_d(a.to_words()), _d(a.flatten()[0]), O.count_op2(op, vs[i], vs[j])])]
    na = int(rng.integers(1, nv + 1))
    t = O.agg_and_sub(vs[:na], vs[na:])
    out += [("agg_and_sub", [_d(t.to_words()), _d(t.flatten()[0])])]
    for oc in (False, True):
        out += [(f"agg_or {oc}", _d(O.agg_or(vs, oc).flatten()[0]))]
    sel = [int(x) for x in rng.integers(0, nv, int(rng.integers(1, 40)))]
    oc, an = bool(rng.integers(0, 2)), bool(rng.integers(0, 2))
    t, f = O.agg_shift_right_and([vs[i] for i in sel], oc, an)
    out += [("shift_right_and", [bool(f), _d(t.to_words()), _d(t.flatten()[0])])]
    groups = []
    for _ in range(int(rng.integers(1, 6))):
        a = [int(x) for x in rng.integers(0, nv, int(rng.integers(0, nv + 1)))]
        s_ = [int(x) for x in rng.integers(0, nv, int(rng.integers(0, nv)))]
        groups.append((a, s_))
    g = [([vs[k] for k in a], [vs[k] for k in s_]) for a, s_ in groups]
    out += [("pipeline_counts", [int(x) for x in O.pipeline_counts(g)])]
    res, cnt, ort = O.pipeline_results(g)
    out += [("pipeline_results", [[int(x) for x in cnt], [None if x is None else [_d(x.to_words()), _d(x.flatten()[0])] for x in res],
                                  _d(ort.to_words()), _d(ort.flatten()[0])])]
    for k, (a, s_) in enumerate(groups):
        if not a: continue
        # the port's fused find_first_and_sub, the reference's find_first over its AND-SUB result; a position only when found
        f, pos = (O.find_first(O.agg_and_sub([vs[m] for m in a], [vs[m] for m in s_])) if O.is_ref
                  else O.find_first_and_sub([vs[m] for m in a], [vs[m] for m in s_]))
        out += [(f"find_first {k}", [bool(f), int(pos) if f else None])]
    rs = O.rs_build(vs[0])
    ql = rng.integers(0, nblk * 65536, 20).astype(np.uint64); qr = rng.integers(0, nblk * 65536, 20).astype(np.uint64)
    for l_, r_ in zip(ql, qr):
        out += [(f"count_range {l_} {r_}", rs.count_range(int(l_), int(r_)))]
        # the reference's rank_corrected / count_to_test read rs_idx.rcount(nb - 1) unchecked: they crash for positions
        # beyond the last block the index knows (trailing empty blocks) -- a precondition, not a result to reproduce
        if int(l_) >> 16 <= _last_nonempty(ws[0]):
            out += [(f"rank_corrected {l_}", [rs.rank_corrected(int(l_)), rs.count_to_test(int(l_))])]
    q = rng.integers(0, nblk * 65536, 50).astype(np.uint64)
    out += [("rank", _d(rs.rank(q)))]
    c = vs[0].count()
    if c:
        r = rng.integers(1, c + 1, 50).astype(np.uint64)
        a, b = rs.select(r)
        out += [("select", [_d(a), _d(b)])]
    return out


def first_difference(got, exp):
    """-> None, or a message naming the first entry where two transcripts part"""
    got = [[k, v] for k, v in got]
    for i, (g, e) in enumerate(zip(got, exp)):
        if g != list(e):
            return f"entry {i}: got {g}, expected {list(e)}"
    if len(got) != len(exp):
        return f"{len(got)} entries, expected {len(exp)}"
    return None


def main():
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    import oracle
    port = oracle.port()
    out = {"reference": oracle.reference("avx2").name, "vs_reference": {}, "soak_seeds": SOAK_SEEDS}
    for flavour in ("scalar", "avx2"):
        out["vs_reference"][flavour] = vs_reference(oracle.reference(flavour), port)
    out["soak"] = [soak_seed(oracle.reference("avx2"), s) for s in range(SOAK_SEEDS)]
    with open(FIXTURE, "w") as f:
        json.dump(out, f, separators=(",", ":"))
        f.write("\n")
    print("wrote", FIXTURE, os.path.getsize(FIXTURE), "bytes")


if __name__ == "__main__":
    main()
