"""mn_graph_dfs / Graph.dfs / Graph.dfs_batch on the device against tests/dfs_model.py — the reference's item stack as it is
written, not the frame form the kernel runs; tests/test_dfs_model.py holds it to the reference's recorded
rows — and against those recorded rows.  Every comparison is equality of whole (node, depth, parent) rows in order.  The
shapes sit on what the kernel switches on: list lengths around the 64-entry chunk, chunks that are visited as a whole, the
out/in boundary inside a chunk, a node named twice in one chunk, stack depths around the wavefront and far beyond, the depth
rule, chunk boundaries of a batch."""
import numpy as np
import pytest

import bfs_model as bm
import dfs_model as dm
from test_bfs_model import bfs_queries, graph_cases
from test_dfs_model import golden

pytestmark = pytest.mark.gpu

DIRECTIONS = ("forward", "reverse", "both")
UNLIMITED = 2**31 - 1


def make(gpu, n, src, dst, w=None):
    return gpu.graph.graph_from_edges(n, src, dst, w), dm.lists_of(n, src, dst)


def check(g, lists, seeds, max_depth, direction):
    got = g.dfs_batch(seeds, max_depth, direction)
    want = dm.dfs_arrays(lists[0], lists[1], seeds, max_depth, direction)
    for name, a, b in zip(("row_off", "node", "depth", "parent"), got, want):
        assert np.array_equal(a, b), (name, len(seeds), max_depth, direction)
    assert g.dfs_stats["rows"] == len(want[1])
    row_off, node = got[0], got[1]
    for i in range(len(seeds)):  # no node twice in a seed's rows: asserted apart from the model
        mine = node[row_off[i]:row_off[i + 1]]
        assert len(np.unique(mine)) == len(mine), (i, max_depth, direction)
    return got


def rows_of(got):
    return list(zip(*(a.tolist() for a in got[-3:])))


def scratch_mb(slots, n, max_depth):
    """an MN_DFS_SCRATCH_MB that admits `slots` seeds per chunk (include/muninn_hip.h: per seed 12 bytes per node, 4 per 32 nodes,
    8 per frame)"""
    per_slot = 12 * n + 4 * ((n + 31) // 32) + 8 * min(n, max_depth)
    return repr((slots + 0.5) * per_slot / 2**20)


# ───────────────────────── the recorded rows ─────────────────────────

@pytest.mark.parametrize("name", sorted(graph_cases()))
def test_recorded_cases(gpu, name):
    ids, index, out, inn = bm.text_graph([(str(s), str(d)) for s, d in graph_cases()[name]])
    g = gpu.Graph(len(ids), *bm.csr_of(out), None, *bm.csr_of(inn), None)
    for (start, max_depth, direction), want in zip(bfs_queries()[name], golden()["dfs"][name]):
        if start not in index:
            continue  # (the SQL layer's case: tests/test_dfs_sql.py)
        node, depth, parent = g.dfs(index[start], max_depth, direction)
        got = [[ids[v], d, None if p < 0 else ids[p]] for v, d, p in zip(node.tolist(), depth.tolist(), parent.tolist())]
        assert got == want, (name, start, max_depth, direction)
    g.close()


# ───────────────────────── the 64-entry chunk ─────────────────────────

@pytest.mark.parametrize("degree", [0, 1, 2, 63, 64, 65, 127, 128, 129, 1025, 5000])
def test_chunk_edges(gpu, degree):
    """one node whose `degree` entries are all fresh: the leaves in reverse list order"""
    g, lists = make(gpu, degree + 1, np.zeros(degree, np.int64), np.arange(1, degree + 1))
    for direction in ("forward", "both"):
        node, depth, parent = check(g, lists, [0], 100, direction)[1:]
        assert node.tolist() == [0] + list(range(degree, 0, -1))
        assert depth.tolist() == [0] + [1] * degree and parent.tolist() == [-1] + [0] * degree
        assert g.dfs_stats["chunks"] == 1 and g.dfs_stats["max_frames"] == (0 if degree == 0 else 1 if direction == "forward" else 2)
    assert g.dfs_stats["entries_scanned"] == 2 * degree  # 'both': the hub's list, and each leaf's one entry (the hub again)
    g.close()


@pytest.mark.parametrize("r", [0, 1, 63, 64, 65, 128, 199, 200])
def test_whole_chunk_skips(gpu, r):
    """a hub (node 0) with entries 0 .. 199 = nodes 1 .. 200, and a chain 200 → 199 → … through the hub's last r entries: when
    the cursor comes back to the hub those r are visited, and the next visit is entry 199 - r, or none"""
    src, dst = [0] * 200, list(range(1, 201))
    for k in range(200, 200 - r + 1, -1):
        src.append(k)
        dst.append(k - 1)
    g, lists = make(gpu, 201, src, dst)
    rows = rows_of(check(g, lists, [0], 1000, "forward"))
    assert len(rows) == 201
    chain = max(r, 1)
    assert rows[1:1 + chain] == [(200 - i, 1 + i, 0 if i == 0 else 201 - i) for i in range(chain)]
    if chain < 200:
        assert rows[1 + chain] == (200 - chain, 1, 0)  # entry 199 - r
    check(g, lists, [0, 200, 100], 1000, "both")
    check(g, lists, [0], 100, "forward")  # the chain cut at depth 100 where it is longer
    g.close()


@pytest.mark.parametrize("d_out,d_in", [(63, 1), (64, 1), (1, 64), (65, 65), (0, 5), (5, 0)])
def test_out_in_boundary_under_both(gpu, d_out, d_in):
    """node 0 with d_out fresh out-entries and d_in fresh in-entries: the in-list's last entry first, the out-list's first last"""
    outs, ins = list(range(1, 1 + d_out)), list(range(1 + d_out, 1 + d_out + d_in))
    g, lists = make(gpu, 1 + d_out + d_in, [0] * d_out + ins, outs + [0] * d_in)
    node, depth, parent = check(g, lists, [0], 100, "both")[1:]
    assert node.tolist() == [0] + ins[::-1] + outs[::-1]
    check(g, lists, [0, 1, d_out + d_in], 100, "forward")
    check(g, lists, [0, 1, d_out + d_in], 100, "reverse")
    g.close()


@pytest.mark.parametrize("case", ["twice_no_way_on", "twice_way_back", "seventy_times", "self_loops", "two_cycle", "twice_across_chunks"])
def test_immediate_revisit(gpu, case):
    """a node named again right below the entry that has just marked it: the second entry is read two round trips after the mark"""
    src, dst = {
        "twice_no_way_on": ([0, 0, 0, 0], [1, 2, 3, 3]),
        "twice_way_back": ([0, 0, 0, 0, 3], [1, 2, 3, 3, 0]),
        "seventy_times": ([0] * 72 + [2], [1] + [2] * 70 + [3] + [0]),
        "self_loops": ([0, 0, 0, 1, 1, 2], [0, 1, 0, 1, 2, 2]),
        "two_cycle": ([0, 1, 0, 1], [1, 0, 1, 0]),
        "twice_across_chunks": ([0] * 130, [1] * 63 + [2] * 4 + [1] * 63),
    }[case]
    n = max(max(src), max(dst)) + 1
    g, lists = make(gpu, n, src, dst)
    for direction in DIRECTIONS:
        for max_depth in (1, 2, 100):
            got = check(g, lists, list(range(n)), max_depth, direction)
            assert len(got[1]) <= n * n
    g.close()


# ───────────────────────── the stack ─────────────────────────

@pytest.mark.parametrize("L", [1, 31, 32, 33, 63, 64, 65, 2000])
def test_frame_depth(gpu, L):
    """a path 0 → 1 → … → L and a leaf L + 1 that the root lists FIRST: it is visited last, after every frame has been popped"""
    leaf = L + 1
    g, lists = make(gpu, L + 2, [0] + list(range(L)), [leaf] + list(range(1, L + 1)))
    for max_depth in (UNLIMITED, L - 1, L, L + 1):
        rows = rows_of(check(g, lists, [0], max_depth, "forward"))
        assert g.dfs_stats["max_frames"] == min(L, max(max_depth, 0)), (L, max_depth)
        if max_depth >= 1:
            assert rows[-1] == (leaf, 1, 0) and len(rows) == min(L, max_depth) + 2
    check(g, lists, [0, L, leaf], UNLIMITED, "both")
    check(g, lists, [L], UNLIMITED, "reverse")
    g.close()


def test_a_node_first_reached_at_max_depth_blocks_the_shallow_way(gpu):
    """0 lists x, then p1; p1 → p2 → x; x → y; x → 0.  p1 is listed last and goes first: x is reached at depth 3, and with
    max_depth 3 it is marked and not expanded, the root's own entry for x finds it visited, and y is never reached — a
    breadth-first traversal has x at depth 1 and y at depth 2"""
    x, p1, p2, y = 1, 2, 3, 4
    g, lists = make(gpu, 5, [0, 0, p1, p2, x, x], [x, p1, p2, x, y, 0])
    assert rows_of(check(g, lists, [0], 3, "forward")) == [(0, 0, -1), (p1, 1, 0), (p2, 2, p1), (x, 3, p2)]
    assert rows_of(check(g, lists, [0], 4, "forward")) == [(0, 0, -1), (p1, 1, 0), (p2, 2, p1), (x, 3, p2), (y, 4, x)]
    assert rows_of(check(g, lists, [0], 2, "forward")) == [(0, 0, -1), (p1, 1, 0), (p2, 2, p1), (x, 1, 0), (y, 2, x)]
    assert [r[:2] for r in bm.bfs(lists[0], lists[1], 0, 3, "forward")] == [(0, 0), (x, 1), (p1, 1), (y, 2), (p2, 2)]
    for direction in DIRECTIONS:
        for max_depth in (1, 2, 3, 4):
            check(g, lists, [0, x, p2], max_depth, direction)
    g.close()


def _random_graph(n, rows, seed, isolated=1):
    rng = np.random.default_rng(seed)
    s, d = rng.integers(0, n - isolated, rows), rng.integers(0, n - isolated, rows)
    s[:40] = d[:40]  # self-loops
    s[40:200], d[40:200] = s[-160:], d[-160:]  # rows that occur twice
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
            assert got[2].max() <= max_depth and g.dfs_stats["max_frames"] <= max_depth


@pytest.mark.parametrize("direction", DIRECTIONS)
def test_random_graph(random3000, direction):
    g, lists, _ = random3000
    seeds = np.random.default_rng(6).integers(0, 2999, 10)
    most = deepest = 0
    for s in seeds:
        node, depth, parent = check(g, lists, [int(s)], UNLIMITED, direction)[1:]
        most, deepest = max(most, len(node)), max(deepest, int(depth.max()))
        want_entries = sum((len(lists[0][v]) if direction != "reverse" else 0) + (len(lists[1][v]) if direction != "forward" else 0)
                           for v in node.tolist())
        stats = g.dfs_stats
        assert stats["entries_scanned"] == want_entries and stats["chunks"] == 1 and stats["device_ms"] > 0
    assert most > 1000 and deepest > 100  # (far deeper than the breadth-first levels of the same graph)
    node, depth, parent = check(g, lists, [2999], 100, direction)[1:]  # no row names it
    assert node.tolist() == [2999]


def test_weights_are_ignored(gpu, random3000):
    g, lists, (s, d) = random3000
    gw, _ = make(gpu, 3000, s, d, np.random.default_rng(8).random(len(s)) + 0.5)
    for direction in DIRECTIONS:
        a, b = g.dfs_batch([3, 1500], 100, direction), gw.dfs_batch([3, 1500], 100, direction)
        assert all(np.array_equal(x, y) for x, y in zip(a, b))
    gw.close()


# ───────────────────────── batches ─────────────────────────

@pytest.fixture(scope="module")
def random600(gpu):
    s, d = _random_graph(600, 2400, 9, isolated=3)
    g, lists = make(gpu, 600, s, d)
    singles = {}

    def single(seed, max_depth, direction):
        key = (seed, max_depth, direction)
        if key not in singles:
            singles[key] = g.dfs(seed, max_depth, direction)
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
@pytest.mark.parametrize("slots", [1, 7, 64])
def test_chunked_batch_is_the_same(random600, monkeypatch, slots, max_depth):
    """a scratch budget of `slots` seeds at once: the chunk count the header's formula gives, the last chunk partial, the same rows"""
    g, lists, _ = random600
    count = {1: 5, 7: 65, 64: 300}[slots]
    seeds = _seeds(count)
    want_chunks = -(-count // slots)
    assert slots == 1 or count % slots
    for direction in ("forward", "both"):
        monkeypatch.delenv("MN_DFS_SCRATCH_MB", raising=False)
        whole = g.dfs_batch(seeds, max_depth, direction)
        assert g.dfs_stats["chunks"] == 1
        monkeypatch.setenv("MN_DFS_SCRATCH_MB", scratch_mb(slots, 600, max_depth))
        parts = check(g, lists, seeds, max_depth, direction)
        assert g.dfs_stats["chunks"] == want_chunks
        assert all(np.array_equal(a, b) for a, b in zip(whole, parts))
    monkeypatch.setenv("MN_DFS_SCRATCH_MB", "0")  # no budget at all: one seed at a time
    check(g, lists, seeds[:5], max_depth, "both")
    assert g.dfs_stats["chunks"] == 5


def test_handle_reuse(gpu, random3000, monkeypatch):
    """a larger, then a smaller graph on fresh handles; one handle at two depth limits and two chunkings; mn_graph_bfs and
    mn_graph_dfs interleaved on one handle, each keeping the rows of its own last call"""
    big, big_lists, _ = random3000
    check(big, big_lists, [5, 77, 5], 100, "both")
    s, d = _random_graph(600, 2400, 9, isolated=3)
    g, lists = make(gpu, 600, s, d)
    first = check(g, lists, [5, 77, 5, 300], 100, "both")
    check(g, lists, list(range(0, 600, 7)), 2, "forward")
    monkeypatch.setenv("MN_DFS_SCRATCH_MB", scratch_mb(10, 600, 100))
    check(g, lists, list(range(0, 600, 7)), 100, "reverse")
    monkeypatch.delenv("MN_DFS_SCRATCH_MB")
    again = check(g, lists, [5, 77, 5, 300], 100, "both")
    assert all(np.array_equal(a, b) for a, b in zip(first, again))
    # the two traversals' rows are apart
    L = gpu.lib()
    bfs = g.bfs_batch([5, 300], 100, "both")
    dfs = check(g, lists, [77], 3, "forward")
    out = [np.empty(len(bfs[1]), np.int32) for _ in range(3)]
    assert L.mn_graph_bfs_rows(g.h, *out) == 0 and all(np.array_equal(a, b) for a, b in zip(out, bfs[1:]))
    assert all(np.array_equal(a, b) for a, b in zip(g.bfs_batch([77], 3, "forward"), bm.bfs_arrays(lists[0], lists[1], [77], 3, "forward")))
    out = [np.empty(len(dfs[1]), np.int32) for _ in range(3)]
    assert L.mn_graph_dfs_rows(g.h, *out) == 0 and all(np.array_equal(a, b) for a, b in zip(out, dfs[1:]))
    g.close()


# ───────────────────────── errors ─────────────────────────

def test_errors_leave_the_handle_usable(gpu):
    s, d = _random_graph(600, 2400, 9, isolated=3)
    g, lists = make(gpu, 600, s, d)
    L = gpu.lib()
    row_off = np.zeros(8, np.int64)
    seeds = np.array([1, 2, 3], np.int32)

    def raw(direction, n_seeds, arr):
        return L.mn_graph_dfs(g.h, direction, n_seeds, arr.ctypes.data, 100, row_off, None)

    for bad in (600, -1, 2**31 - 1):
        assert raw(1, 3, np.array([1, bad, 3], np.int32)) == -1
        assert "seed" in gpu.graph._gerr()
        out = [np.empty(4, np.int32) for _ in range(3)]
        assert L.mn_graph_dfs_rows(g.h, *out) == -1  # a failed call leaves no rows
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
            g.dfs(1, 100, direction)
        node, depth, parent = g.dfs(1, 100, "forward")
        assert list(zip(node.tolist(), depth.tolist(), parent.tolist())) == dm.dfs(lists[0], lists[1], 1, 100, "forward")
    g.close()


def test_every_host_allocation_fails_cleanly(gpu):
    """tests/test_fault_inject.py's walk over one mn_graph_dfs call: -1 and a message at every allocation, never an exception
    through the C frame, and the same handle gives the same answer afterwards"""
    s, d = _random_graph(600, 2400, 9, isolated=3)
    L = gpu.lib()
    seeds = list(range(0, 600, 5))
    g, lists = make(gpu, 600, s, d)  # a fresh handle: the first call also allocates the handle's traversal state
    L.mn_debug_fault_alloc(0)
    want = g.dfs_batch(seeds, 100, "both")
    total = L.mn_debug_fault_alloc(0)
    g.close()
    assert total >= 1
    failed = 0
    for nth in range(1, total + 1):
        g, _ = make(gpu, 600, s, d)
        L.mn_debug_fault_alloc(0)
        L.mn_debug_fault_alloc(nth)
        try:
            g.dfs_batch(seeds, 100, "both")
        except gpu.MuninnHipError as e:
            failed += 1
            assert "memory" in str(e) or "exception" in str(e), str(e)
        finally:
            L.mn_debug_fault_alloc(0)
        got = g.dfs_batch(seeds, 100, "both")
        assert all(np.array_equal(a, b) for a, b in zip(want, got)), nth
        g.close()
    assert failed >= max(1, total // 2), (failed, total)
