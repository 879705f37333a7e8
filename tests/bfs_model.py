"""The reference's run_bfs (src/graph_tvf.c:230-309) in plain Python over adjacency lists: a queue, a visited set, a node's
out-list before its in-list, each in table-row order, the popped node as parent of what it discovers, no expansion at
max_depth.  The checker for shapes too large to record from the compiled reference (tests/test_bfs.py, bench_bfs.py);
tests/test_bfs_model.py holds it to the recorded rows."""
from collections import deque

import numpy as np


def lists_of(n, src, dst):
    """(out lists, in lists) of an edge list with integer node indices, each list in row order"""
    out, inn = [[] for _ in range(n)], [[] for _ in range(n)]
    for s, d in zip(np.asarray(src).tolist(), np.asarray(dst).tolist()):
        out[s].append(d)
        inn[d].append(s)
    return out, inn


def csr_of(lists):
    """(off int32[n + 1], tgt int32[E]) of adjacency lists"""
    off = np.zeros(len(lists) + 1, np.int64)
    off[1:] = np.cumsum([len(x) for x in lists])
    tgt = np.fromiter((v for x in lists for v in x), np.int32, int(off[-1]))
    return off.astype(np.int32), tgt


def bfs(out, inn, seed, max_depth=100, direction="forward"):
    """→ [(node, depth, parent)] in queue order; parent is -1 for the seed.  A direction other than the three follows no list."""
    fwd, rev = direction in ("forward", "both"), direction in ("reverse", "both")
    seen = {seed}
    q = deque([(seed, 0, -1)])
    rows = []
    while q:
        u, d, p = q.popleft()
        rows.append((u, d, p))
        if d < max_depth:
            for use, lists in ((fwd, out), (rev, inn)):
                if use:
                    for v in lists[u]:
                        if v not in seen:
                            seen.add(v)
                            q.append((v, d + 1, u))
    return rows


def bfs_arrays(out, inn, seeds, max_depth=100, direction="forward"):
    """bfs for every seed → (row_off int64, node, depth, parent int32), the layout of Graph.bfs_batch"""
    off, rows = [0], []
    for s in seeds:
        rows += bfs(out, inn, int(s), max_depth, direction)
        off.append(len(rows))
    a = np.asarray(rows, np.int32).reshape(-1, 3)
    return np.asarray(off, np.int64), a[:, 0].copy(), a[:, 1].copy(), a[:, 2].copy()


def trace(rows, start, end):
    """run_shortest_path_bfs's trace (src/graph_tvf.c:541-572) through a forward BFS's rows: the path start .. end, or []"""
    up = {v: p for v, _, p in rows}
    if end not in up:
        return []
    path = [end]
    while path[-1] != start:
        path.append(up[path[-1]])
    return path[::-1]


def text_graph(rows):
    """a table's (src, dst) text rows → (ids in first-seen order, index of each id, out lists, in lists); a row with a NULL
    endpoint is skipped"""
    index, ids, src, dst = {}, [], [], []
    for s, d in rows:
        if s is None or d is None:
            continue
        for x in (s, d):
            if x not in index:
                index[x] = len(ids)
                ids.append(x)
        src.append(index[s])
        dst.append(index[d])
    return (ids, index) + lists_of(len(ids), src, dst)


def text_bfs(rows, start, max_depth=100, direction="forward"):
    """graph_bfs's rows over a table of text ids → [[node, depth, parent or None]]"""
    ids, index, out, inn = text_graph([(None if s is None else str(s), None if d is None else str(d)) for s, d in rows])
    if start not in index:
        return [[start, 0, None]]
    return [[ids[v], d, None if p < 0 else ids[p]] for v, d, p in bfs(out, inn, index[start], max_depth, direction)]


def text_path(rows, start, end):
    """graph_shortest_path's node column (no weight_col) over a table of text ids"""
    ids, index, out, inn = text_graph([(str(s), str(d)) for s, d in rows])
    if start not in index:
        return [start] if start == end else []
    if end not in index:
        return []
    return [ids[v] for v in trace(bfs(out, inn, index[start], 2**31 - 1, "forward"), index[start], index[end])]
