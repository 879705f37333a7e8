"""The reference's run_dfs (src/graph_tvf.c:322-416) in plain Python over adjacency lists, AS THE REFERENCE WRITES IT: a stack
of (node, depth, parent) items, a visited set, an item dropped when it is popped and its node is visited, a node's unvisited
neighbours pushed (out-list before in-list, each in table-row order) while depth < max_depth.  Not the frame form the device
runs: tests/test_dfs.py checks that restatement against this, not against a copy of itself.  The checker for
shapes too large to record from the compiled reference (tests/test_dfs.py, bench_dfs.py); tests/test_dfs_model.py holds it to
the recorded rows."""
import numpy as np

from bfs_model import csr_of, lists_of, text_graph  # noqa: F401  (the same graphs as the BFS model's)


def run_dfs(out, inn, seed, max_depth=100, direction="forward"):
    """→ [(node, depth, parent)] in pop order; parent is -1 for the seed.  A direction other than the three follows no list."""
    fwd, rev = direction in ("forward", "both"), direction in ("reverse", "both")
    visited = set()
    stack = [(seed, 0, -1)]
    rows = []
    while stack:
        u, d, p = stack.pop()
        if u in visited:
            continue
        visited.add(u)
        rows.append((u, d, p))
        if d < max_depth:
            for use, lists in ((fwd, out), (rev, inn)):
                if use:
                    for v in lists[u]:
                        if v not in visited:
                            stack.append((v, d + 1, u))
    return rows


dfs = run_dfs


def dfs_arrays(out, inn, seeds, max_depth=100, direction="forward"):
    """dfs for every seed → (row_off int64, node, depth, parent int32), the layout of Graph.dfs_batch"""
    off, rows = [0], []
    for s in seeds:
        rows += run_dfs(out, inn, int(s), max_depth, direction)
        off.append(len(rows))
    a = np.asarray(rows, np.int32).reshape(-1, 3)
    return np.asarray(off, np.int64), a[:, 0].copy(), a[:, 1].copy(), a[:, 2].copy()


def text_dfs(rows, start, max_depth=100, direction="forward"):
    """graph_dfs's rows over a table of text ids → [[node, depth, parent or None]]"""
    ids, index, out, inn = text_graph([(None if s is None else str(s), None if d is None else str(d)) for s, d in rows])
    if start not in index:
        return [[start, 0, None]]
    return [[ids[v], d, None if p < 0 else ids[p]] for v, d, p in run_dfs(out, inn, index[start], max_depth, direction)]
