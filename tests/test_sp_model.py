"""tests/sp_model.py against what the compiled reference's graph_shortest_path returned, with a weight column, for the cases
below (tests/golden/shortest_path.json.gz, written by scripts/gen_sp_golden.py).  CPU only: the model is the checker of
tests/test_shortest_path.py and bench_sp.py for shapes that are not recorded, so it is itself held to the recorded rows here.
Distances are compared as the hex text of their f64."""
import gzip
import json
import os

import numpy as np
import pytest

import sp_model as sm

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "shortest_path.json.gz")
INF = float("inf")


def golden():
    with gzip.open(GOLDEN, "rb") as f:
        return json.loads(f.read().decode())


def _random_rows(n, rows, seed, weight):
    rng = np.random.default_rng(seed)
    s, d = rng.integers(0, n, rows), rng.integers(0, n, rows)
    return [(f"n{a}", f"n{b}", weight(rng)) for a, b in zip(s.tolist(), d.tolist())]


def graph_cases():
    """name → the (src, dst, weight) rows of an edge table, in row order"""
    cases = {
        # tie-heavy: integer weights 1..3
        "ties": _random_rows(40, 170, 11, lambda r: float(r.integers(1, 4))),
        # weights 0..2: zero-weight edges and (40 nodes, 170 rows) zero-weight cycles
        "zeros": _random_rows(40, 170, 12, lambda r: float(r.integers(0, 3))),
        "reals": _random_rows(40, 170, 13, lambda r: float(r.random()) + 0.01),
        "infinite": _random_rows(30, 110, 15, lambda r: INF if r.random() < 0.3 else float(r.integers(1, 5))),
    }
    # two rows that occur twice, with the same and with another weight, and self-loops
    dups = _random_rows(30, 100, 14, lambda r: float(r.integers(1, 4)))
    dups += [dups[3], (dups[5][0], dups[5][1], 0.5), ("n1", "n1", 0.0), ("n2", "n2", 1.0), dups[7]]
    cases["duplicates"] = dups
    # a negative weight: b is reached at 1 and settled before the cheaper way through c is seen; the reference keeps what it settled
    cases["negative"] = [("a", "b", 1.0), ("a", "c", 2.0), ("c", "b", -3.0), ("b", "d", 1.0), ("c", "d", 5.0), ("d", "e", -0.5),
                         ("a", "e", 2.25), ("e", "f", 1.0)]
    # a zero-weight cycle on the way, and two equal ways round it
    cases["zero_cycle"] = [("s", "a", 1.0), ("a", "b", 0.0), ("b", "c", 0.0), ("c", "a", 0.0), ("s", "c", 1.0), ("c", "t", 2.0),
                           ("b", "t", 2.0), ("t", "t", 0.0), ("lonely", "s", 1.0)]
    return cases


def path_queries():
    """name → [(start, end)]"""
    q = {name: [("n0", "n7"), ("n7", "n33" if name != "infinite" and name != "duplicates" else "n23"), ("n3", "n0"), ("n5", "n20"),
                ("n1", "n19"), ("n19", "n1"), ("n12", "n4"), ("n9", "n9"), ("n2", "n28"), ("n28", "n2"), ("n10", "n17"),
                ("n6", "n25"), ("n0", "nowhere"), ("nowhere", "nowhere")]
         for name in ("ties", "zeros", "reals", "infinite", "duplicates")}
    q["negative"] = [("a", "d"), ("a", "b"), ("a", "e"), ("a", "f"), ("c", "e"), ("f", "a"), ("b", "b")]
    q["zero_cycle"] = [("s", "t"), ("s", "b"), ("a", "t"), ("b", "a"), ("t", "s"), ("s", "lonely"), ("lonely", "t")]
    return q


def hexed(rows):
    return [[node, float(d).hex()] for node, d in rows]


@pytest.mark.parametrize("name", sorted(graph_cases()))
def test_model_equals_the_recorded_rows(name):
    rows, z = graph_cases()[name], golden()["paths"][name]
    assert len(z) == len(path_queries()[name])
    for (start, end), want in zip(path_queries()[name], z):
        assert hexed(sm.text_path(rows, start, end)) == want, (name, start, end)


def test_recorded_grid_is_not_vacuous():
    z = golden()["paths"]
    every = [p for case in z.values() for p in case]
    assert sum(len(p) >= 4 for p in every) >= 10 and sum(len(p) == 0 for p in every) >= 5
    assert any(r[1] == INF.hex() for p in z["infinite"] for r in p), "no recorded distance is infinite"
    # the negative weight: the reference answers 2.0 for a → d, not the -1 + 1 = 0 a correct search would find
    assert z["negative"][0] == [["a", (0.0).hex()], ["b", (1.0).hex()], ["d", (2.0).hex()]]
    assert golden()["ambiguous"] >= 1


def test_canonical_rule_on_the_zero_weight_cycle():
    """a, b and c are all at distance 1; c is one edge from s, a too, b two: the canonical path to t takes c (fewest edges),
    and the tight BFS ends although a → b → c → a is tight all the way round"""
    ids, index, out = sm.text_graph(graph_cases()["zero_cycle"])
    nodes, dists = sm.canonical(out, index["s"], index["t"])
    assert [ids[v] for v in nodes] == ["s", "c", "t"] and dists == [0.0, 1.0, 3.0]
    nodes, _ = sm.canonical(out, index["s"], index["b"])
    assert [ids[v] for v in nodes] == ["s", "a", "b"]
    dist = sm.distances(out, index["s"])
    assert not sm.unambiguous(sm.tight_predecessors(out, dist), dist, index["s"], index["t"])


@pytest.mark.parametrize("name", ["ties", "zeros", "reals", "infinite", "duplicates", "zero_cycle"])
def test_fixpoint_distances_equal_the_recorded_ones(name):
    """the claim the fast mode rests on: with weights >= 0 the fixpoint is what the reference settles, bit for bit, and an
    unambiguous path is the reference's"""
    rows, z = graph_cases()[name], golden()["paths"][name]
    ids, index, out = sm.text_graph(rows)
    for (start, end), want in zip(path_queries()[name], z):
        if start not in index or end not in index or start == end:
            continue
        dist = sm.distances(out, index[start])
        assert (dist[index[end]] is None) == (want == [])
        for node, d in want:
            assert dist[index[node]].hex() == d, (name, start, end, node)
        if want and sm.unambiguous(sm.tight_predecessors(out, dist), dist, index[start], index[end]):
            assert hexed([[ids[v], d] for v, d in zip(*sm.canonical(out, index[start], index[end], dist))]) == want
