"""mn_graph_shortest_paths / Graph.shortest_paths on the device.  Replay mode against the rows recorded from the compiled
reference (tests/golden/shortest_path.json.gz) and against tests/sp_model.py (itself held to those rows by
tests/test_sp_model.py) at the shapes its kernel switches on; fast mode against the model's fixpoint distances and its
canonical path, under three values of delta and two chunkings; the unweighted half against the paths recorded in
tests/golden/bfs.json.gz.  Every comparison is equality: node lists, and the bits of every f64."""
import functools

import numpy as np
import pytest

import bfs_model as bm
import sp_model as sm
import test_bfs_model as tb
from test_sp_model import golden, graph_cases, path_queries

pytestmark = pytest.mark.gpu

INF = float("inf")
DELTAS = ("1e-9", None, "inf")  # tiny: a threshold move per distinct distance; the default; plain frontier Bellman-Ford


def make(gpu, n, src, dst, w):
    return gpu.graph.graph_from_edges(n, src, dst, w), sm.lists_of(n, src, dst, w)


def paths_of(res):
    """Graph.shortest_paths's answer → [(node list, hex distance list)] per pair"""
    row_off, node, dist = res
    return [(node[a:b].tolist(), [d.hex() for d in dist[a:b].tolist()]) for a, b in zip(row_off[:-1].tolist(), row_off[1:].tolist())]


def hexed(nodes, dists):
    return nodes, [float(d).hex() for d in dists]


def random_graph(n, rows, seed, weight):
    rng = np.random.default_rng(seed)
    s, d = rng.integers(0, n, rows), rng.integers(0, n, rows)
    return s, d, np.array([weight(rng) for _ in range(rows)], np.float64)


# ───────────────────────── replay: the recorded rows ─────────────────────────

@pytest.mark.parametrize("mode", ["replay", "auto"])
@pytest.mark.parametrize("name", sorted(graph_cases()))
def test_replay_equals_the_recorded_rows(gpu, name, mode):
    ids, index, out = sm.text_graph(graph_cases()[name])
    src = [u for u, lst in enumerate(out) for _ in lst]
    g, _ = make(gpu, len(ids), src, [v for lst in out for v, _ in lst], [w for lst in out for _, w in lst])
    asked = [(q, want) for q, want in zip(path_queries()[name], golden()["paths"][name]) if q[0] in index and q[1] in index]
    assert len(asked) >= 5
    got = paths_of(g.shortest_paths([index[q[0]] for q, _ in asked], [index[q[1]] for q, _ in asked], mode=mode))
    assert g.sp_stats["mode_used"] == gpu.graph.SP_REPLAY  # auto: every case is far below MN_SP_REPLAY_MAX
    for (q, want), (nodes, dists) in zip(asked, got):
        assert [[ids[v], d] for v, d in zip(nodes, dists)] == want, (name, q)
    g.close()


# ───────────────────────── replay: the model, where the kernel can go wrong ─────────────────────────

def check_replay(g, out, pairs):
    got = paths_of(g.shortest_paths([p[0] for p in pairs], [p[1] for p in pairs], mode="replay"))
    total = dict(pops=0, pushes=0)
    for (s, e), have in zip(pairs, got):
        st = {}
        assert have == hexed(*sm.replay(out, s, e, st)), (s, e)
        total["pops"] += st["pops"]
        total["pushes"] += st["pushes"]
    assert g.sp_stats["pops"] == total["pops"] and g.sp_stats["pushes"] == total["pushes"]
    return got


@functools.lru_cache(maxsize=None)
def tie_heavy():
    """300 nodes, 3 000 rows, weights 1..3: queues of hundreds of entries, most of them tied"""
    return random_graph(300, 3000, 21, lambda r: float(r.integers(1, 4)))


def test_replay_queue_past_128_entries_with_ties_in_every_stride(gpu):
    s, d, w = tie_heavy()
    g, out = make(gpu, 300, s, d, w)
    pairs = [(int(a), int(b)) for a, b in np.random.default_rng(5).integers(0, 300, (24, 2))]
    st = {}
    sm.replay(out, *pairs[0], st)
    # the queue passes 64 and 128 entries, minima are taken far beyond the first stride, entries go stale
    assert st["max_queue"] > 128 and st["max_min_index"] >= 128 and st["stale"] > 0
    check_replay(g, out, pairs)
    g.close()


def test_replay_lists_longer_than_a_wavefront_and_equal_minima(gpu):
    """s → 200 leaves, all at 1.0 (equal minima in every lane and in four strides; each pop moves the last entry into the
    hole), the leaves → t and → one another; a second hub whose newest entry is the minimum"""
    src, dst, w = [], [], []
    leaves = list(range(2, 202))
    for v in leaves:
        src += [0, v, v]
        dst += [v, 1, 2 + (v * 7) % 200]
        w += [1.0, 1.0 + (v % 3), 0.0]
    src += [202, 202, 203]
    dst += [203, 204, 1]
    w += [5.0, 1.0, 1.0]  # 202's queue is [203 at 5, 204 at 1]: the minimum is the last entry
    src += [204] * 70
    dst += [203] * 70
    w += [3.0 - 0.01 * i for i in range(70)]  # 70 entries for one node: 69 stale pops unless the end comes first
    g, out = make(gpu, 205, src, dst, w)
    assert len(out[0]) == 200 and len(out[204]) == 70
    st = {}
    sm.replay(out, 202, 1, st)
    assert st["last_pops"] >= 1 and st["stale"] >= 60
    check_replay(g, out, [(0, 1), (0, 150), (202, 204), (202, 1), (202, 203), (5, 0), (1, 1)])
    g.close()


def test_replay_in_three_chunks_equals_one_chunk(gpu, monkeypatch):
    s, d, w = tie_heavy()
    g, out = make(gpu, 300, s, d, w)
    pairs = np.random.default_rng(6).integers(0, 300, (200, 2))
    one = g.shortest_paths(pairs[:, 0], pairs[:, 1], mode="replay")
    assert g.sp_stats["chunks"] == 1 and g.sp_stats["sources"] == 200
    per_pair = 16 * (len(s) + 1) + 12 * 300
    monkeypatch.setenv("MN_SP_SCRATCH_MB", repr(per_pair * 70.5 / 1048576))
    many = g.shortest_paths(pairs[:, 0], pairs[:, 1], mode="replay")
    assert g.sp_stats["chunks"] == 3
    for a, b in zip(one, many):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8))
    for i in (0, 71, 199):  # and the one-chunk answer is the model's
        assert paths_of(one)[i] == hexed(*sm.replay(out, int(pairs[i, 0]), int(pairs[i, 1])))
    g.close()


def test_replay_refuses_nan_and_takes_negative_weights(gpu):
    g, out = make(gpu, 3, [0, 1], [1, 2], [1.0, float("nan")])
    with pytest.raises(gpu.graph.MuninnHipError, match="NaN"):
        g.shortest_path(0, 2, mode="replay")
    g.close()
    g, out = make(gpu, 4, [0, 0, 2, 1], [1, 2, 1, 3], [1.0, 2.0, -3.0, 1.0])
    assert paths_of(g.shortest_paths([0], [3], mode="auto"))[0] == hexed(*sm.replay(out, 0, 3))
    assert g.sp_stats["mode_used"] == gpu.graph.SP_REPLAY
    with pytest.raises(gpu.graph.MuninnHipError, match="fast mode needs weights >= 0"):
        g.shortest_path(0, 3, mode="fast")
    g.close()


# ───────────────────────── fast ─────────────────────────

@functools.lru_cache(maxsize=None)
def fast_case(kind):
    """(n, src, dst, w, starts, ends): 6 starts with 6 ends each (one of them the start itself)"""
    n = 1000
    weight = {"reals": lambda r: float(r.random()) + 1e-3, "ties": lambda r: float(r.integers(1, 4)),
              "zeros": lambda r: float(r.integers(0, 3)), "infinite": lambda r: INF if r.random() < 0.3 else float(r.integers(1, 5))}[kind]
    s, d, w = random_graph(n, 5000, {"reals": 31, "ties": 32, "zeros": 33, "infinite": 34}[kind], weight)
    rng = np.random.default_rng(41)
    starts = np.repeat(rng.choice(n, 6, replace=False), 6)
    ends = rng.integers(0, n, 36)
    ends[::6] = starts[::6]
    order = rng.permutation(36)  # the pairs of a start do not stand together
    return n, s, d, w, starts[order], ends[order]


@functools.lru_cache(maxsize=None)
def fast_model(kind):
    """per pair: (canonical path, hex distances, whether it is the only shortest path), and the model's distances per start"""
    n, s, d, w, starts, ends = fast_case(kind)
    out = sm.lists_of(n, s, d, w)
    per_start = {}
    for a in set(starts.tolist()):
        dist = sm.distances(out, a)
        per_start[a] = (dist, sm.tight_levels(out, dist, a), sm.tight_predecessors(out, dist))
    rows = []
    for a, b in zip(starts.tolist(), ends.tolist()):
        dist, tree, pred = per_start[a]
        rows.append((hexed(*sm.canonical(out, a, b, dist, tree)), sm.unambiguous(pred, dist, a, b)))
    return out, per_start, rows


def fast_runs(gpu, monkeypatch, kind):
    """the case under every delta and two chunkings (all starts in one launch; one start per launch) → the answers"""
    n, s, d, w, starts, ends = fast_case(kind)
    g, _ = make(gpu, n, s, d, w)
    runs = []
    for delta in DELTAS:
        for scratch in (None, repr(40 * n * 1.5 / 1048576)):
            for var, val in (("MN_SSSP_DELTA", delta), ("MN_SP_SCRATCH_MB", scratch)):
                monkeypatch.setenv(var, val) if val else monkeypatch.delenv(var, raising=False)
            runs.append(g.shortest_paths(starts, ends, mode="fast"))
            assert g.sp_stats["mode_used"] == gpu.graph.SP_FAST and g.sp_stats["sources"] == 6
            assert g.sp_stats["chunks"] == (6 if scratch else 1)
    monkeypatch.delenv("MN_SSSP_DELTA", raising=False)
    monkeypatch.delenv("MN_SP_SCRATCH_MB", raising=False)
    replayed = paths_of(g.shortest_paths(starts, ends, mode="replay"))
    g.close()
    return runs, replayed


@pytest.mark.parametrize("kind", ["reals", "ties", "zeros", "infinite"])
def test_fast_mode(gpu, monkeypatch, kind):
    """distances: the model's bits on every traced node, under every delta and chunking.  Rows: identical under all of them;
    on every pair each step is tight, the path has the fewest edges and is the canonical one (the model's); where the model
    finds one shortest path only, the rows are replay's, which are the reference's."""
    n, s, d, w, starts, ends = fast_case(kind)
    out, per_start, want = fast_model(kind)
    runs, replayed = fast_runs(gpu, monkeypatch, kind)
    for other in runs[1:]:
        for a, b in zip(runs[0], other):
            assert np.array_equal(a.view(np.uint8), b.view(np.uint8))
    got = paths_of(runs[0])
    only = 0
    for i, (a, b) in enumerate(zip(starts.tolist(), ends.tolist())):
        dist, (level, _), _ = per_start[a]
        nodes, dists = got[i]
        assert (nodes == []) == (dist[b] is None), (kind, a, b)
        assert dists == [dist[v].hex() for v in nodes], (kind, a, b)
        if nodes:
            assert nodes[0] == a and nodes[-1] == b and len(nodes) == level[b] + 1  # fewest edges among the shortest
            for u, v in zip(nodes, nodes[1:]):
                assert any(t == v and dist[u] + x == dist[v] for t, x in out[u]), (kind, a, b, u, v)
        assert (nodes, dists) == want[i][0], (kind, a, b)
        assert replayed[i][1][-1:] == dists[-1:]  # the reference's distance, ambiguous or not
        if want[i][1]:
            only += len(nodes) > 1
            assert (nodes, dists) == replayed[i], (kind, a, b)
    found = sum(1 for p in got if len(p[0]) > 1)
    assert found >= 12
    if kind == "reals":
        assert 2 * only >= found  # the comparison with replay is not vacuous
    if kind in ("ties", "zeros"):
        assert only < found  # and neither is the canonical rule: some pair has more than one shortest path


def test_fast_wide_frontiers_and_a_hub(gpu, monkeypatch):
    """root → 300 nodes (a list of 300; frontiers past 64 and 256 entries) → 300 nodes, each reached from two → a sink"""
    width, a0, b0, end = 300, 1, 301, 601
    src, dst, w = [], [], []
    for i in range(width):
        src += [0, a0 + i, a0 + i]
        dst += [a0 + i, b0 + (i + 1) % width, b0 + i]
        w += [1.0 + (i % 5), 2.0, 2.0 + (i % 2)]
    src += list(range(b0, b0 + width))
    dst += [end] * width
    w += [1.0] * width
    g, out = make(gpu, end + 1, src, dst, w)
    ends = [end, b0, b0 + 150, a0 + 299, 0]
    dist = sm.distances(out, 0)
    tree = sm.tight_levels(out, dist, 0)
    for delta in DELTAS:
        monkeypatch.setenv("MN_SSSP_DELTA", delta) if delta else monkeypatch.delenv("MN_SSSP_DELTA", raising=False)
        got = paths_of(g.shortest_paths([0] * len(ends), ends, mode="fast"))
        assert got == [hexed(*sm.canonical(out, 0, e, dist, tree)) for e in ends], delta
        assert g.sp_stats["sources"] == 1 and g.sp_stats["relaxations"] >= 300
    g.close()


def test_fast_stops_once_its_ends_are_final(gpu, monkeypatch):
    """a path of 2 000 nodes: with delta = 1 the search for node 5 ends after a few threshold moves, while almost every
    node is still unreached; run to the end (delta = inf) it gives the same rows"""
    n = 2000
    g, out = make(gpu, n, np.arange(n - 1), np.arange(1, n), np.ones(n - 1))
    monkeypatch.setenv("MN_SSSP_DELTA", "1")
    early = g.shortest_paths([0, 0], [5, 3], mode="fast")
    assert g.sp_stats["passes"] < 40
    assert paths_of(early) == [hexed(list(range(6)), [float(i) for i in range(6)]), hexed(list(range(4)), [float(i) for i in range(4)])]
    monkeypatch.setenv("MN_SSSP_DELTA", "inf")
    late = g.shortest_paths([0, 0], [5, 3], mode="fast")
    assert g.sp_stats["passes"] >= n - 1
    for a, b in zip(early, late):
        assert np.array_equal(a, b)
    monkeypatch.setenv("MN_SSSP_DELTA", "1")
    assert paths_of(g.shortest_paths([7, 1999], [1999, 7], mode="fast")) == [hexed(list(range(7, n)), [float(i) for i in range(n - 7)]), ([], [])]
    g.close()


# ───────────────────────── unweighted, and the interface ─────────────────────────

@pytest.mark.parametrize("name", sorted(tb.graph_cases()))
def test_unweighted_equals_the_recorded_bfs_paths(gpu, name):
    ids, index, out, inn = bm.text_graph([(str(s), str(d)) for s, d in tb.graph_cases()[name]])
    off, tgt = bm.csr_of(out)
    asked = [(q, want) for q, want in zip(tb.path_queries()[name], tb.golden()["paths"][name]) if q[0] in index and q[1] in index]
    for weights, weighted in ((None, True), (None, False), (np.full(len(tgt), 2.5), False)):
        g = gpu.Graph(len(ids), off, tgt, weights, *bm.csr_of(inn), weights)
        got = paths_of(g.shortest_paths([index[q[0]] for q, _ in asked], [index[q[1]] for q, _ in asked], weighted=weighted))
        assert g.sp_stats["mode_used"] == gpu.graph.SP_UNWEIGHTED
        for (q, want), (nodes, dists) in zip(asked, got):
            assert [ids[v] for v in nodes] == want and dists == [float(i).hex() for i in range(len(want))], (name, q)
        g.close()


def test_interface_edges(gpu):
    g, out = make(gpu, 4, [0, 1], [1, 2], [1.5, 2.5])
    row_off, node, dist = g.shortest_paths([], [])
    assert row_off.tolist() == [0] and len(node) == 0
    for mode in ("replay", "fast"):
        assert paths_of(g.shortest_paths([3, 0, 2, 0], [3, 2, 0, 0], mode=mode)) == [
            ([3], [(0.0).hex()]), ([0, 1, 2], [(0.0).hex(), (1.5).hex(), (4.0).hex()]), ([], []), ([0], [(0.0).hex()])]
    n2, d2 = g.shortest_path(0, 2)
    assert n2.tolist() == [0, 1, 2] and d2.tolist() == [0.0, 1.5, 4.0]
    for bad in ([4], [-1]):
        with pytest.raises(gpu.graph.MuninnHipError, match="outside 0 .. 3"):
            g.shortest_paths([0], bad)
    g.close()


@pytest.mark.parametrize("mode, weighted", [("replay", True), ("fast", True), ("auto", False)])
def test_every_host_allocation_fails_cleanly(gpu, mode, weighted):
    """tests/test_fault_inject.py's walk over one mn_graph_shortest_paths call: -1 and a message at every allocation, never an
    exception through the C frame, and the same handle gives the same answer afterwards"""
    s, d, w = random_graph(200, 900, 51, lambda r: float(r.integers(1, 4)))
    L = gpu.lib()
    pairs = np.random.default_rng(52).integers(0, 200, (30, 2))
    g, _ = make(gpu, 200, s, d, w)  # a fresh handle: the first call also allocates the handle's state
    L.mn_debug_fault_alloc(0)
    want = g.shortest_paths(pairs[:, 0], pairs[:, 1], weighted=weighted, mode=mode)
    total = L.mn_debug_fault_alloc(0)
    g.close()
    assert total >= 1
    failed = 0
    for nth in range(1, total + 1):
        g, _ = make(gpu, 200, s, d, w)
        L.mn_debug_fault_alloc(0)
        L.mn_debug_fault_alloc(nth)
        try:
            g.shortest_paths(pairs[:, 0], pairs[:, 1], weighted=weighted, mode=mode)
        except gpu.MuninnHipError as e:
            failed += 1
            assert "memory" in str(e) or "exception" in str(e), str(e)
        finally:
            L.mn_debug_fault_alloc(0)
        got = g.shortest_paths(pairs[:, 0], pairs[:, 1], weighted=weighted, mode=mode)
        assert all(np.array_equal(a.view(np.uint8), b.view(np.uint8)) for a, b in zip(want, got)), nth
        g.close()
    assert failed >= max(1, total // 2), (failed, total)


def test_auto_replays_small_and_negative_graphs_only(gpu, monkeypatch):
    """MN_SP_AUTO: replay up to MN_SP_REPLAY_MAX - 1 list entries (4 095 unless the variable says otherwise), fast beyond —
    unless a weight is negative, which only replay takes"""
    s, d, w = random_graph(300, 4095, 61, lambda r: float(r.integers(1, 4)))
    g, out = make(gpu, 300, s, d, w)
    want = hexed(*sm.replay(out, 1, 200))
    assert paths_of(g.shortest_paths([1], [200]))[0] == want and g.sp_stats["mode_used"] == gpu.graph.SP_REPLAY
    g.close()
    s, d, w = np.append(s, 0), np.append(d, 1), np.append(w, 1.0)
    g, out = make(gpu, 300, s, d, w)
    dist = sm.distances(out, 1)
    got = paths_of(g.shortest_paths([1], [200]))[0]
    assert g.sp_stats["mode_used"] == gpu.graph.SP_FAST and got == hexed(*sm.canonical(out, 1, 200, dist))
    monkeypatch.setenv("MN_SP_REPLAY_MAX", "5000")
    assert paths_of(g.shortest_paths([1], [200]))[0] == hexed(*sm.replay(out, 1, 200)) and g.sp_stats["mode_used"] == gpu.graph.SP_REPLAY
    monkeypatch.delenv("MN_SP_REPLAY_MAX")
    g.close()
    w[7] = -0.5
    g, out = make(gpu, 300, s, d, w)
    assert paths_of(g.shortest_paths([1], [200]))[0] == hexed(*sm.replay(out, 1, 200)) and g.sp_stats["mode_used"] == gpu.graph.SP_REPLAY
    g.close()
