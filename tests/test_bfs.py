"""mn_graph_bfs / Graph.bfs / Graph.bfs_batch on the device against tests/bfs_model.py (itself held to the reference's
recorded rows by tests/test_bfs_model.py) and against those recorded rows.  Every comparison is equality of whole
(node, depth, parent) rows in order.  The shapes sit on what the kernels switch on: list lengths around the wavefront, the
workgroup and the 2 048-edge range of the counting pass, frontier widths around the same, claims contested by hundreds of
edges, thousands of levels, chunk boundaries."""
import numpy as np
import pytest

import bfs_model as bm
from test_bfs_model import bfs_queries, golden, graph_cases

pytestmark = pytest.mark.gpu

DIRECTIONS = ("forward", "reverse", "both")
UNLIMITED = 2**31 - 1


def make(gpu, n, src, dst, w=None):
    return gpu.graph.graph_from_edges(n, src, dst, w), bm.lists_of(n, src, dst)


def check(g, lists, seeds, max_depth, direction):
    got = g.bfs_batch(seeds, max_depth, direction)
    want = bm.bfs_arrays(lists[0], lists[1], seeds, max_depth, direction)
    for name, a, b in zip(("row_off", "node", "depth", "parent"), got, want):
        assert np.array_equal(a, b), (name, len(seeds), max_depth, direction)
    assert g.bfs_stats["rows"] == len(want[1])
    return got


# ───────────────────────── the recorded rows ─────────────────────────

@pytest.mark.parametrize("name", sorted(graph_cases()))
def test_recorded_cases(gpu, name):
    ids, index, out, inn = bm.text_graph([(str(s), str(d)) for s, d in graph_cases()[name]])
    g = gpu.Graph(len(ids), *bm.csr_of(out), None, *bm.csr_of(inn), None)
    for (start, max_depth, direction), want in zip(bfs_queries()[name], golden()["bfs"][name]):
        if start not in index:
            continue  # (the SQL layer's case: tests/test_bfs_sql.py)
        node, depth, parent = g.bfs(index[start], max_depth, direction)
        got = [[ids[v], d, None if p < 0 else ids[p]] for v, d, p in zip(node.tolist(), depth.tolist(), parent.tolist())]
        assert got == want, (name, start, max_depth, direction)
    z = golden()["paths"][name]
    from test_bfs_model import path_queries

    for (start, end), want in zip(path_queries()[name], z):
        if start in index and end in index:
            assert [ids[v] for v in g.shortest_path_unweighted(index[start], index[end])] == want, (name, start, end)
    g.close()


# ───────────────────────── list lengths ─────────────────────────

@pytest.mark.parametrize("degree", [0, 1, 2, 63, 64, 65, 255, 256, 257, 1023, 1025, 5000])
def test_hub_degrees(gpu, degree):
    """a hub whose list has `degree` entries with duplicates among them, expanded as the seed and as the LAST entry of a
    300-node frontier whose other members reach for the same targets"""
    rng = np.random.default_rng(degree)
    root, hub, t0 = 0, 300, 301
    T = max(2, degree // 2 + 3)
    sink = t0 + T
    src, dst = [], []
    for i in range(1, 300):
        src += [root, i, i]
        dst += [i, t0 + i * 7 % T, t0 + i * 13 % T]
    src.append(root)
    dst.append(hub)
    src += [hub] * degree
    dst += (t0 + rng.integers(0, T, degree)).tolist()
    src += list(range(t0, t0 + T))
    dst += [sink] * T
    g, lists = make(gpu, sink + 1, src, dst)
    assert len(lists[0][hub]) == degree and (degree < 4 or len(set(lists[0][hub])) < degree)
    for direction in ("forward", "both"):
        check(g, lists, [hub], 100, direction)
        node, depth, parent = check(g, lists, [root], 100, direction)[1:]
        assert node[300] == hub and depth[300] == 1  # the last of the 300
    g.close()


@pytest.mark.parametrize("width", [1, 63, 64, 65, 256, 257, 4097])
def test_frontier_widths(gpu, width):
    """root → `width` nodes → `width` nodes (each reached from two of the level before) → one node"""
    a0, b0, end = 1, 1 + width, 1 + 2 * width
    src, dst = [], []
    for i in range(width):
        src += [0, a0 + i, a0 + i]
        dst += [a0 + (i * 5 + 3) % width if np.gcd(5, width) == 1 else a0 + i, b0 + (i + 1) % width, b0 + i]
    src += list(range(b0, b0 + width))
    dst += [end] * width
    g, lists = make(gpu, end + 1, src, dst)
    for direction in DIRECTIONS:
        row_off, node, depth, parent = check(g, lists, [0, end], 100, direction)
    got = g.bfs(0, 100, "forward")
    assert np.bincount(got[1]).tolist() == [1, width, width, 1]
    g.close()


def test_contested_claims(gpu):
    """300 x 300 all-to-all between two levels, every list in an order of its own: the parent of each of the 300 is the
    first of the frontier and nothing else, and they stand in the order of ITS list"""
    rng = np.random.default_rng(11)
    a0, b0 = 1, 301
    src, dst = [0] * 300, list(range(a0, a0 + 300))
    for i in range(300):
        src += [a0 + i] * 300
        dst += (b0 + rng.permutation(300)).tolist()
    g, lists = make(gpu, 601, src, dst)
    node, depth, parent = check(g, lists, [0], 100, "forward")[1:]
    assert (parent[301:] == a0).all() and node[301:].tolist() == lists[0][a0]
    check(g, lists, [0, 5, 600], 100, "both")
    check(g, lists, [600, 450], 100, "reverse")
    g.close()


# ───────────────────────── depth ─────────────────────────

def test_two_thousand_levels(gpu):
    n = 2000
    g, lists = make(gpu, n, np.arange(n - 1), np.arange(1, n))
    node, depth, parent = check(g, lists, [0], UNLIMITED, "forward")[1:]
    assert len(node) == n and depth[-1] == n - 1 and g.bfs_stats["levels"] == n and g.bfs_stats["edges_scanned"] == n - 1
    node, depth, parent = check(g, lists, [0], 1000, "forward")[1:]
    assert len(node) == 1001 and g.bfs_stats["levels"] == 1000
    assert g.shortest_path_unweighted(3, 1500) == list(range(3, 1501)) and g.shortest_path_unweighted(1500, 3) == []
    check(g, lists, [1999, 1000], UNLIMITED, "reverse")
    check(g, lists, [1000], UNLIMITED, "both")
    g.close()


def _random_graph(n, rows, seed, isolated=1):
    rng = np.random.default_rng(seed)
    s, d = rng.integers(0, n - isolated, rows), rng.integers(0, n - isolated, rows)
    s[:40] = d[:40]  # self-loops
    s[40:200], d[40:200] = s[-160:], d[-160:]  # duplicates
    return s, d


@pytest.fixture(scope="module")
def random3000(gpu):
    s, d = _random_graph(3000, 12000, 5)
    g, lists = make(gpu, 3000, s, d)
    yield g, lists, (s, d)
    g.close()


@pytest.mark.parametrize("max_depth", [0, 1, 2, 100, -1])
def test_depth_limits(random3000, max_depth):
    g, lists, _ = random3000
    for direction in DIRECTIONS:
        got = check(g, lists, [17, 2000, 17], max_depth, direction)
        if max_depth <= 0:
            assert got[1].tolist() == [17, 2000, 17] and got[3].tolist() == [-1, -1, -1]
        else:
            assert got[2].max() <= max_depth


@pytest.mark.parametrize("direction", DIRECTIONS)
def test_random_graph(random3000, direction):
    g, lists, _ = random3000
    seeds = np.random.default_rng(6).integers(0, 2999, 10)
    most = 0
    for s in seeds:
        node, depth, parent = check(g, lists, [int(s)], 100, direction)[1:]
        most = max(most, len(node))
        want_edges = sum((len(lists[0][v]) if direction != "reverse" else 0) + (len(lists[1][v]) if direction != "forward" else 0)
                         for v, d in zip(node.tolist(), depth.tolist()) if d < 100)
        stats = g.bfs_stats
        assert stats["edges_scanned"] == want_edges and stats["chunks"] == 1 and stats["device_ms"] > 0
    assert most > 1000
    node, depth, parent = check(g, lists, [2999], 100, direction)[1:]  # no row names it
    assert node.tolist() == [2999]


def test_weights_are_ignored(gpu, random3000):
    g, lists, (s, d) = random3000
    gw, _ = make(gpu, 3000, s, d, np.random.default_rng(8).random(len(s)) + 0.5)
    for direction in DIRECTIONS:
        a, b = g.bfs_batch([3, 1500], 100, direction), gw.bfs_batch([3, 1500], 100, direction)
        assert all(np.array_equal(x, y) for x, y in zip(a, b))
    gw.close()


def test_pool_grows_in_the_middle_of_a_traversal(random3000, monkeypatch):
    """450 seeds in one chunk whose rows outnumber the pool's first allocation, so the pool is grown between two levels
    with the rows so far kept.  That rests on mn_bfs.hip's first pool size, min(S * N, max(64 * S, 2^20)) entries: 2^20 here,
    where S * N is 1 350 000 and no earlier call on this handle has had more than a few seeds.  The same seeds 100 to a
    chunk (300 000 entries: no growth) give the same rows."""
    g, lists, _ = random3000
    seeds = list(range(0, 2700, 6))
    assert len(seeds) == 450
    monkeypatch.delenv("MN_BFS_SCRATCH_MB", raising=False)
    whole = check(g, lists, seeds, UNLIMITED, "both")
    stats = g.bfs_stats
    print("pool growth: chunks", stats["chunks"], "rows", stats["rows"], "levels", stats["levels"])
    assert stats["chunks"] == 1
    assert stats["rows"] > 2**20
    monkeypatch.setenv("MN_BFS_SCRATCH_MB", repr((100 + 0.5) * 64 * 3000 / 2**20))
    parts = g.bfs_batch(seeds, UNLIMITED, "both")
    assert g.bfs_stats["chunks"] == 5
    assert all(np.array_equal(a, b) for a, b in zip(whole, parts))


# ───────────────────────── batches ─────────────────────────

@pytest.fixture(scope="module")
def random600(gpu):
    s, d = _random_graph(600, 2400, 9, isolated=3)
    g, lists = make(gpu, 600, s, d)
    singles = {}

    def single(seed, max_depth, direction):
        key = (seed, max_depth, direction)
        if key not in singles:
            singles[key] = g.bfs(seed, max_depth, direction)
        return singles[key]

    yield g, lists, single
    g.close()


def _seeds(count):
    s = np.random.default_rng(count).integers(0, 600, count)
    s[count // 2:] = s[:count - count // 2]  # repeats
    return s


@pytest.mark.parametrize("max_depth", [1, 2, 100])
@pytest.mark.parametrize("count", [1, 2, 63, 64, 65, 300])
def test_batch_equals_single_calls_and_the_model(random600, count, max_depth):
    g, lists, single = random600
    seeds = _seeds(count)
    for direction in ("forward", "both"):
        row_off, node, depth, parent = check(g, lists, seeds, max_depth, direction)
        for i, s in enumerate(seeds.tolist()):
            one = single(s, max_depth, direction)
            for a, b in zip((node, depth, parent), one):
                assert np.array_equal(a[row_off[i]:row_off[i + 1]], b), (count, max_depth, direction, i)


@pytest.mark.parametrize("max_depth", [1, 2, 100])
@pytest.mark.parametrize("count", [63, 65, 300])
def test_chunked_batch_is_the_same(random600, monkeypatch, count, max_depth):
    """a scratch budget of `slots` seeds at once (include/muninn_hip.h: 64 bytes per node per seed): at least three chunks, the
    last one partial, and the same rows"""
    g, lists, _ = random600
    seeds = _seeds(count)
    slots = {63: 25, 65: 32, 300: 128}[count]
    want_chunks = -(-count // slots)
    assert want_chunks >= 3 and count % slots
    for direction in ("forward", "both"):
        monkeypatch.delenv("MN_BFS_SCRATCH_MB", raising=False)
        whole = g.bfs_batch(seeds, max_depth, direction)
        assert g.bfs_stats["chunks"] == 1
        monkeypatch.setenv("MN_BFS_SCRATCH_MB", repr((slots + 0.5) * 64 * 600 / 2**20))
        parts = check(g, lists, seeds, max_depth, direction)
        assert g.bfs_stats["chunks"] == want_chunks
        assert all(np.array_equal(a, b) for a, b in zip(whole, parts))
    monkeypatch.setenv("MN_BFS_SCRATCH_MB", "0")  # no budget at all: one seed at a time
    check(g, lists, seeds[:5], max_depth, "both")
    assert g.bfs_stats["chunks"] == 5


def test_handle_reuse(gpu, monkeypatch):
    """A, then B, then A again on one handle: what a chunk touched in the visited words is what is reset after it"""
    s, d = _random_graph(600, 2400, 9, isolated=3)
    g, lists = make(gpu, 600, s, d)
    runs = [([5, 77, 5, 300], 100, "both"), (list(range(0, 600, 7)), 2, "forward"), ([5, 77, 5, 300], 100, "both"),
            ([599], 100, "reverse"), (list(range(0, 600, 7)), 100, "reverse"), ([5, 77, 5, 300], 100, "both")]
    first = None
    for i, (seeds, max_depth, direction) in enumerate(runs):
        if i == 4:
            monkeypatch.setenv("MN_BFS_SCRATCH_MB", repr(10.5 * 64 * 600 / 2**20))
        got = check(g, lists, seeds, max_depth, direction)
        if direction == "both":
            first = first or got
            assert all(np.array_equal(a, b) for a, b in zip(first, got))
    g.close()


# ───────────────────────── errors ─────────────────────────

def test_errors_leave_the_handle_usable(gpu):
    s, d = _random_graph(600, 2400, 9, isolated=3)
    g, lists = make(gpu, 600, s, d)
    L = gpu.lib()
    row_off = np.zeros(8, np.int64)
    seeds = np.array([1, 2, 3], np.int32)

    def raw(direction, n_seeds, arr):
        return L.mn_graph_bfs(g.h, direction, n_seeds, arr.ctypes.data, 100, row_off, None)

    for bad in (600, -1, 2**31 - 1):
        assert raw(1, 3, np.array([1, bad, 3], np.int32)) == -1
        assert "seed" in gpu.graph._gerr()
        check(g, lists, [1, 2], 100, "forward")
    assert raw(1, -1, seeds) == -1 and "n_seeds" in gpu.graph._gerr()
    assert raw(3, 3, seeds) == -1 and "direction" in gpu.graph._gerr()
    assert raw(1, 0, seeds) == 0 and row_off[0] == 0
    check(g, lists, [1, 2], 100, "both")
    g.close()
    # a graph loaded for one direction only has no answer for the others
    off_out, tgt_out = bm.csr_of(lists[0])
    none = np.zeros(601, np.int32)
    g = gpu.Graph(600, off_out, tgt_out, None, none, np.zeros(1, np.int32), None)
    for direction in ("reverse", "both"):
        with pytest.raises(gpu.MuninnHipError, match="does not hold"):
            g.bfs(1, 100, direction)
        node, depth, parent = g.bfs(1, 100, "forward")
        want = bm.bfs(lists[0], lists[1], 1, 100, "forward")
        assert [list(r) for r in zip(node.tolist(), depth.tolist(), parent.tolist())] == [list(r) for r in want]
    g.close()


def test_every_host_allocation_fails_cleanly(gpu):
    """tests/test_fault_inject.py's walk over one mn_graph_bfs call: -1 and a message at every allocation, never an exception
    through the C frame, and the same handle gives the same answer afterwards"""
    s, d = _random_graph(600, 2400, 9, isolated=3)
    L = gpu.lib()
    seeds = list(range(0, 600, 5))
    g, lists = make(gpu, 600, s, d)  # a fresh handle: the first call also allocates the handle's traversal state
    L.mn_debug_fault_alloc(0)
    want = g.bfs_batch(seeds, 100, "both")
    total = L.mn_debug_fault_alloc(0)
    g.close()
    assert total >= 1
    failed = 0
    for nth in range(1, total + 1):
        g, _ = make(gpu, 600, s, d)
        L.mn_debug_fault_alloc(0)
        L.mn_debug_fault_alloc(nth)
        try:
            g.bfs_batch(seeds, 100, "both")
        except gpu.MuninnHipError as e:
            failed += 1
            assert "memory" in str(e) or "exception" in str(e), str(e)
        finally:
            L.mn_debug_fault_alloc(0)
        got = g.bfs_batch(seeds, 100, "both")
        assert all(np.array_equal(a, b) for a, b in zip(want, got)), nth
        g.close()
    assert failed >= max(1, total // 2), (failed, total)
