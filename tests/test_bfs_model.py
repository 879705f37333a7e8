"""tests/bfs_model.py against what the compiled reference's graph_bfs and graph_shortest_path returned for the cases below
(tests/golden/bfs.json.gz, written by scripts/gen_bfs_golden.py).  CPU only: the model is the checker of tests/test_bfs.py and
bench_bfs.py for shapes too large to record, so it is itself held to the recorded rows here."""
import gzip
import json
import os

import numpy as np
import pytest

import bfs_model as bm

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bfs.json.gz")
DIRECTIONS = ("forward", "reverse", "both")


def golden():
    with gzip.open(GOLDEN, "rb") as f:
        return json.loads(f.read().decode())


def _random_rows(n, rows, seed, loops, dups):
    rng = np.random.default_rng(seed)
    s, d = rng.integers(0, n, rows), rng.integers(0, n, rows)
    s[:loops] = d[:loops]  # self-loops
    s[loops:loops + dups], d[loops:loops + dups] = s[-dups:], d[-dups:]  # rows that occur twice
    return [(f"n{a}", f"n{b}") for a, b in zip(s.tolist(), d.tolist())]


def graph_cases():
    """name → the (src, dst) rows of an edge table, in row order"""
    return {
        # duplicates, a self-loop, a cycle back to the start, a node that only ever appears as a source
        "table": [("a", "c"), ("a", "b"), ("b", "d"), ("c", "d"), ("d", "a"), ("a", "b"), ("a", "a"), ("x", "a"), ("c", "e")],
        "path": [(f"p{i}", f"p{i + 1}") for i in range(9)],
        # t is reached through b and through a: the parent is whichever the queue pops first (b: r's list names it first)
        "diamond": [("r", "b"), ("r", "a"), ("a", "t"), ("b", "t"), ("a", "u"), ("t", "z"), ("u", "z"), ("z", "r")],
        "integers": [(1, 2), (1, 3), (3, 2), (2, 10), (10, 1), (7, 1)],
        "er60": _random_rows(60, 240, 1, 6, 12),
        "er300": _random_rows(300, 1200, 2, 10, 30),
    }


def bfs_queries():
    """name → [(start, max_depth, direction)]"""
    q = {
        "table": [("a", m, d) for d in DIRECTIONS for m in (1, 2, 100)] + [("x", 100, "forward"), ("e", 100, "forward"),
                                                                            ("e", 100, "both"), ("nowhere", 100, "both")],
        "path": [("p0", 100, "forward"), ("p0", 4, "forward"), ("p9", 100, "reverse"), ("p4", 100, "both"), ("p4", 2, "both")],
        "diamond": [("r", 100, d) for d in DIRECTIONS] + [("a", 2, "both")],
        "integers": [("1", 100, d) for d in DIRECTIONS] + [("7", 100, "forward")],
    }
    for name, starts in (("er60", ("n0", "n7", "n33")), ("er300", ("n1", "n150"))):
        q[name] = [(s, m, d) for s in starts for d in DIRECTIONS for m in (1, 2, 100)]
    return q


def path_queries():
    """name → [(start, end)] for graph_shortest_path without a weight column"""
    return {
        "table": [("a", "e"), ("a", "d"), ("x", "e"), ("e", "a"), ("a", "a"), ("a", "nowhere")],
        "path": [("p0", "p9"), ("p3", "p5"), ("p5", "p3")],
        "diamond": [("r", "z"), ("a", "b"), ("u", "t")],
        "integers": [("7", "10"), ("1", "2")],
        "er60": [("n0", "n7"), ("n7", "n33"), ("n33", "n0"), ("n5", "n50")],
        "er300": [("n1", "n150"), ("n150", "n1"), ("n2", "n299")],
    }


@pytest.mark.parametrize("name", sorted(graph_cases()))
def test_model_equals_the_recorded_rows(name):
    rows, z = graph_cases()[name], golden()["bfs"][name]
    assert len(z) == len(bfs_queries()[name])
    for (start, max_depth, direction), want in zip(bfs_queries()[name], z):
        assert bm.text_bfs(rows, start, max_depth, direction) == want, (name, start, max_depth, direction)


@pytest.mark.parametrize("name", sorted(graph_cases()))
def test_parent_trace_equals_the_recorded_shortest_paths(name):
    rows, z = graph_cases()[name], golden()["paths"][name]
    assert len(z) == len(path_queries()[name])
    for (start, end), want in zip(path_queries()[name], z):
        assert bm.text_path(rows, start, end) == want, (name, start, end)


def test_recorded_grid_is_not_vacuous():
    z = golden()["bfs"]
    assert any(max(r[1] for r in rows) >= 3 for case in z.values() for rows in case)
    assert graph_cases()["diamond"].count(("a", "t")) == 1 and z["diamond"][0][3] == ["t", 2, "b"]
