"""The reference's run_shortest_path_dijkstra (src/graph_tvf.c:600-753) in plain Python over out-lists — the array it calls a
priority queue, popped at the first index of the strict minimum, the last entry moved into the hole, stale entries dropped,
unsettled targets appended in list order — and the canonical rule of the library's fast mode: distances are
the fixpoint of dist[v] = min fl(dist[u] + w); the path has the fewest edges among the shortest ones, and every node's parent
is the tight edge from the previous level with the lowest (parent index, place in its list).  The checker for shapes that
are not recorded from the compiled reference (tests/test_shortest_path.py, bench_sp.py); tests/test_sp_model.py holds it to
the recorded rows.  Python's float is the f64 of the reference, and + is its addition."""
from collections import deque


def lists_of(n, src, dst, w):
    """out lists [(target, weight)] of an edge list with integer node indices, each list in row order"""
    out = [[] for _ in range(n)]
    for s, d, x in zip(list(src), list(dst), list(w)):
        out[int(s)].append((int(d), float(x)))
    return out


def replay(out, start, end, stats=None):
    """→ (nodes, distances) of the reference's path, start first; ([], []) when end is never settled.  stats, a dict, receives
    pops, pushes, stale (popped entries whose node was settled), max_queue, max_min_index (the largest index a pop took) and
    last_pops (pops that took the last entry)."""
    q = [(start, 0.0, None)]
    settled = {}
    st = dict(pops=0, pushes=0, stale=0, max_queue=1, max_min_index=0, last_pops=0)
    found = False
    while q and not found:
        m = 0
        for i in range(1, len(q)):
            if q[i][1] < q[m][1]:
                m = i
        st["max_min_index"] = max(st["max_min_index"], m)
        st["last_pops"] += m == len(q) - 1 and len(q) > 1
        u, du, par = q[m]
        q[m] = q[-1]
        q.pop()
        st["pops"] += 1
        if u in settled:
            st["stale"] += 1
            continue
        settled[u] = (du, par)
        if u == end:
            found = True
            break
        for v, w in out[u]:
            if v not in settled:
                q.append((v, du + w, u))
                st["pushes"] += 1
        st["max_queue"] = max(st["max_queue"], len(q))
    if stats is not None:
        stats.update(st)
    if not found:
        return [], []
    nodes, dists = [], []
    x = end
    while x is not None:
        nodes.append(x)
        dists.append(settled[x][0])
        x = settled[x][1]
    return nodes[::-1], dists[::-1]


def distances(out, start):
    """the fixpoint, weights >= 0: dist[v] or None where start does not reach v (a label-correcting queue; any order gives
    the same floats)"""
    dist = [None] * len(out)
    dist[start] = 0.0
    q, queued = deque([start]), {start}
    while q:
        u = q.popleft()
        queued.discard(u)
        for v, w in out[u]:
            nd = dist[u] + w
            if dist[v] is None or nd < dist[v]:
                dist[v] = nd
                if v not in queued:
                    queued.add(v)
                    q.append(v)
    return dist


def tight_levels(out, dist, start):
    """the BFS over tight edges → (level, parent) per node, None where start does not reach it"""
    n = len(out)
    level, parent = [None] * n, [None] * n
    level[start] = 0
    frontier = [start]
    while frontier:
        claim = {}
        for u in sorted(frontier):  # (parent index, place in its list) ascending: the first claim is the least
            for j, (v, w) in enumerate(out[u]):
                if level[v] is None and dist[v] is not None and dist[u] + w == dist[v] and v not in claim:
                    claim[v] = u
        for v, u in claim.items():
            level[v] = level[u] + 1
            parent[v] = u
        frontier = list(claim)
    return level, parent


def canonical(out, start, end, dist=None, tree=None):
    """→ (nodes, distances) of the fast mode's path, or ([], [])"""
    dist = dist or distances(out, start)
    if dist[end] is None:
        return [], []
    level, parent = tree or tight_levels(out, dist, start)
    nodes = [end]
    while nodes[-1] != start:
        nodes.append(parent[nodes[-1]])
    nodes.reverse()
    return nodes, [dist[v] for v in nodes]


def tight_predecessors(out, dist):
    """per node the set of OTHER nodes with a tight edge into it"""
    pred = [set() for _ in out]
    for u, lst in enumerate(out):
        if dist[u] is None:
            continue
        for v, w in lst:
            if v != u and dist[u] + w == dist[v]:
                pred[v].add(u)
    return pred


def unambiguous(pred, dist, start, end):
    """whether exactly one shortest path leads from start to end: one tight predecessor at each step back"""
    if dist[end] is None:
        return False
    x, steps = end, 0
    while x != start:
        if len(pred[x]) != 1 or steps > len(pred):
            return False
        x = next(iter(pred[x]))
        steps += 1
    return not pred[start]  # (a zero-weight cycle through the start would offer a second way round)


def text_graph(rows):
    """a table's (src, dst, weight) rows with text ids → (ids in first-seen order, index of each id, out lists)"""
    index, ids, src, dst, w = {}, [], [], [], []
    for s, d, x in rows:
        for k in (s, d):
            if k not in index:
                index[k] = len(ids)
                ids.append(k)
        src.append(index[s])
        dst.append(index[d])
        w.append(x)
    return ids, index, lists_of(len(ids), src, dst, w)


def text_path(rows, start, end):
    """graph_shortest_path's (node, distance) rows with a weight column over a table of text ids"""
    ids, index, out = text_graph(rows)
    if start == end:
        return [[start, 0.0]]
    if start not in index or end not in index:
        return []
    nodes, dists = replay(out, index[start], index[end])
    return [[ids[v], d] for v, d in zip(nodes, dists)]
