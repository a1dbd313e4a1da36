"""CPU: the reference fixture of Kleene three-valued AND / OR over (value, not-NULL) pairs (bm::and_kleene / bm::or_kleene,
src/bm3vl.h:151-262): kleene_ref.json reproduces from the oracle port driven through the reference's eight-step sequence and
from a NumPy model of the per-bit rules, case by case; the scalar truth tables of the reference agree with the model; where
the reference is built, the generator reproduces the committed file.  (The device entries this fixture is for are not in the
library yet.)"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, GOLDEN)
AND, OR, XOR, SUB = 0, 1, 2, 3


def _fixture():
    with open(os.path.join(GOLDEN, "kleene_ref.json")) as f:
        return json.load(f)


def test_fixture_is_small_and_complete():
    assert os.path.getsize(os.path.join(GOLDEN, "kleene_ref.json")) < 100_000
    from kleene_cases import B, case_nbits, cases
    fx = _fixture()["cases"]
    cs = cases()
    assert sorted(fx) == sorted(cs) and len(cs) == 13
    q = cs["every_kind_quadruple"]
    assert case_nbits(q) == 256 * B - 77 and fx["every_kind_quadruple"]["nbits"] == 256 * B - 77
    # block b of (v1, n1, v2, n2) has the kinds (b & 3, b >> 2 & 3, b >> 4 & 3, b >> 6 & 3): all 256 combinations
    for s, key in enumerate(("v1", "n1", "v2", "n2")):
        ids = q["vecs"][key][0]
        held = np.bincount((ids >> np.uint64(16)).astype(np.int64), minlength=256)
        for b in range(256):
            kind = (b >> (2 * s)) & 3
            assert (held[b] == 0) == (kind == 0) and (held[b] >= B - 77) == (kind == 1), (key, b)
    assert np.setdiff1d(q["vecs"]["v1"][0], q["vecs"]["n1"][0]).size > 0                        # v not inside n occurs ...
    i = cs["initialised"]
    assert np.setdiff1d(i["vecs"]["v1"][0], i["vecs"]["n1"][0]).size == 0                       # ... and not after init_kleene
    for c in (fx["every_kind_quadruple"], fx["initialised"]):
        for op in ("and", "or"):
            for out in ("value", "null"):
                assert all(c[op][out]["opt1"]["counts"]), (op, out)                             # every block kind comes out
    # the GAP limit, both sides, in both outputs of both operations: 1,275 runs a GAP block, 1,276 a bit-block
    g = fx["gap_threshold"]
    for op in ("and", "or"):
        for out in ("value", "null"):
            k = g[op][out]["opt1"]["counts"]
            assert k[2] >= 1 and k[3] >= 1, (op, out, k)
    assert g["and"]["value"]["opt1"]["counts"] == [6, 0, 1, 1] and g["or"]["null"]["opt1"]["counts"] == [2, 4, 1, 1]
    assert fx["all_unknown"]["and"]["counts"] == [0, 3 * B, 0] and fx["all_known"]["or"]["counts"][1] == 0
    assert fx["five_bits"]["nbits"] == 5 and sum(fx["five_bits"]["and"]["counts"]) == 5
    assert [fx["fold_%d" % n]["npairs"] for n in (1, 2, 5, 17)] == [1, 2, 5, 17] and fx["fold_3_repeats_a_pair"]["npairs"] == 3
    p = cs["fold_3_repeats_a_pair"]["pairs"]
    assert p[0] == p[2] and cs["value_is_null_vector"]["pairs"][0][0] == cs["value_is_null_vector"]["pairs"][0][1]
    assert sorted({nb for _, nb in cs["ragged_1_3_8"]["vecs"].values()}) == [B, 3 * B - 1000, 3 * B, 8 * B]
    for name, c in fx.items():
        for op in ("and", "or"):
            assert sum(c[op]["counts"]) == c["nbits"], (name, op)
            assert c[op]["counts"][0] + c[op]["counts"][2] == c[op]["null"]["count"], (name, op)


@pytest.mark.parametrize("name", sorted(_fixture()["cases"]))
def test_port_matches_reference_fixture(name, port):
    """the C port through the reference's own eight steps (op2 and nothing else), folded with the in-place form"""
    from kleene_cases import cases, oracle_case
    assert oracle_case(port, cases()[name]) == _fixture()["cases"][name]


@pytest.mark.parametrize("name", sorted(_fixture()["cases"]))
def test_bit_rule_model_matches_reference_fixture(name):
    """no oracle at all: the per-bit rules on unpacked bits, tables from the storage rule"""
    from kleene_cases import model_case
    c = _fixture()["cases"][name]
    m = model_case(name)
    assert m["npairs"] == c["npairs"] and m["nbits"] == c["nbits"]
    for op in ("and", "or"):
        assert m[op]["counts"] == c[op]["counts"], (name, op)
        for out in ("value", "null"):
            for k in ("nbits", "count", "ids_sha", "opt1"):
                assert m[op][out][k] == c[op][out][k], (name, op, out, k)
            k0 = m[op][out]["opt0"]["counts"]
            assert k0[3] == 0 and k0[0] >= c[op][out]["opt1"]["counts"][0]      # without optimize: NULL, FULL or bit-blocks


# and_values_kleene / or_values_kleene (src/bm3vl.h:271-340) restated: rows a = -1, 0, +1 (false, unknown, true), columns b
AND_TABLE = [[-1, -1, -1],
             [-1,  0,  0],
             [-1,  0,  1]]
OR_TABLE = [[-1,  0,  1],
            [ 0,  0,  1],
            [ 1,  1,  1]]


def test_scalar_truth_tables_against_the_bit_rules():
    """the nine combinations as initialised one-bit pairs through the model's pairwise step"""
    from kleene_cases import model_step
    enc = {-1: (False, True), 0: (False, False), 1: (True, True)}              # (v, n), v inside n
    dec = lambda v, n: (1 if v else -1) if n else 0
    a = np.array([enc[x][0] for x in (-1, 0, 1) for _ in range(3)]), np.array([enc[x][1] for x in (-1, 0, 1) for _ in range(3)])
    b = np.array([enc[y][0] for _ in range(3) for y in (-1, 0, 1)]), np.array([enc[y][1] for _ in range(3) for y in (-1, 0, 1)])
    for op, table in ((AND, AND_TABLE), (OR, OR_TABLE)):
        V, N = model_step(op, a[0], a[1], b[0], b[1])
        got = [dec(bool(v), bool(n)) for v, n in zip(V, N)]
        assert got == [table[i][j] for i in range(3) for j in range(3)], (op, got)
        assert not (V & ~N).any() or op == OR                      # AND of initialised pairs stays initialised
    # Kleene's tables are min / max over false < unknown < true
    assert AND_TABLE == [[min(x, y) for y in (-1, 0, 1)] for x in (-1, 0, 1)]
    assert OR_TABLE == [[max(x, y) for y in (-1, 0, 1)] for x in (-1, 0, 1)]


def test_generator_reproduces_fixture_where_the_reference_is_built():
    import oracle
    if not oracle.have_reference("avx2"):
        return                                               # (the committed fixture is what the other tests check)
    r = subprocess.run([sys.executable, os.path.join(GOLDEN, "make_kleene_golden.py"), "--check"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
