"""tests/dfs_model.py against what the compiled reference's graph_dfs returned for the cases and queries of
tests/test_bfs_model.py (tests/golden/dfs.json.gz, written by scripts/gen_dfs_golden.py).  CPU only: the model is the checker
of tests/test_dfs.py and bench_dfs.py for shapes too large to record, so it is itself held to the recorded rows here."""
import functools
import gzip
import json
import os

import pytest

import bfs_model as bm
import dfs_model as dm
from test_bfs_model import bfs_queries, graph_cases

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dfs.json.gz")


@functools.lru_cache(maxsize=None)
def golden():
    with gzip.open(GOLDEN, "rb") as f:
        return json.loads(f.read().decode())


def non_vacuity(recorded):
    """over every recorded traversal, how many: visit the nodes in another order than the BFS of the same query; return fewer
    rows than that BFS under a depth limit below 100; hold a node deeper than its BFS depth; differ, under 'both', from
    'forward'.  The BFS side is tests/bfs_model.py, held to the reference's graph_bfs by tests/test_bfs_model.py."""
    order = fewer = deeper = both = 0
    for name, rows in graph_cases().items():
        by_query = dict(zip(bfs_queries()[name], recorded[name]))
        for (start, max_depth, direction), got in by_query.items():
            bfs = bm.text_bfs(rows, start, max_depth, direction)
            order += [r[0] for r in got] != [r[0] for r in bfs]
            fewer += max_depth < 100 and len(got) < len(bfs)
            at = {r[0]: r[1] for r in bfs}
            deeper += any(r[1] > at[r[0]] for r in got if r[0] in at)
            both += direction == "both" and got != by_query.get((start, max_depth, "forward"), got)
    return order, fewer, deeper, both


@pytest.mark.parametrize("name", sorted(graph_cases()))
def test_model_equals_the_recorded_rows(name):
    rows, z = graph_cases()[name], golden()["dfs"][name]
    assert len(z) == len(bfs_queries()[name])
    for (start, max_depth, direction), want in zip(bfs_queries()[name], z):
        assert dm.text_dfs(rows, start, max_depth, direction) == want, (name, start, max_depth, direction)


def test_recorded_grid_is_not_vacuous():
    order, fewer, deeper, both = non_vacuity(golden()["dfs"])
    assert order > 0, "no traversal's node order differs from BFS's"
    assert fewer > 0, "no depth-limited traversal returns fewer rows than BFS at the same limit"
    assert deeper > 0, "no node is recorded deeper than its BFS depth"
    assert both > 0, "no 'both' case differs from 'forward'"


def test_no_node_twice_in_any_recorded_traversal():
    for case in golden()["dfs"].values():
        for rows in case:
            assert len({r[0] for r in rows}) == len(rows)
