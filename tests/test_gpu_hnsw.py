"""GPU parity tests (-m gpu): the HIP path through the C-ABI vs the CPU oracle on identical seeded
inputs.  Bit-exact for ids, slots, levels and neighbour lists; distances bit-exact against the
oracle running the same summation order, and within 1e-5 relative of the reference order."""
import numpy as np
import pytest

from util import check_topk_f64, gauss, same_bits

pytestmark = pytest.mark.gpu

METRICS = ["l2", "cosine", "inner_product"]


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("dim", [1, 3, 4, 5, 7, 8, 31, 128, 260, 768, 1536, 2500])
def test_dist_batch_bit_exact(gpu, orc, metric, dim):
    X = gauss(200, dim, 7)
    q = gauss(1, dim, 8)[0]
    X[3] = 0.0  # zero vector → cosine 1.0 (src/vec_math.c:122-125)
    X[5] = q  # identical
    for order, oorder in ((gpu.ORDER_SSE, orc.ORDER_SSE), (gpu.ORDER_WAVE, orc.ORDER_WAVE)):
        got = gpu.vec_dist_batch(metric, q, X, order)
        want = orc.dist_batch(metric, q, X, oorder)
        assert same_bits(got, want), (metric, dim, order)
    # fast order vs the reference order: 1e-5 relative (north_star).  "Relative" is taken against the
    # natural scale of the quantity: cosine distance is 1 - cos (absolute accuracy of the subtraction,
    # scale 1); a dot product / squared distance of near-orthogonal or near-identical vectors cancels,
    # so its scale is |q||x| resp. |q|^2 + |x|^2.
    ref = orc.dist_batch(metric, q, X, orc.ORDER_SSE)
    fast = gpu.vec_dist_batch(metric, q, X, gpu.ORDER_WAVE)
    qn, xn = np.linalg.norm(q), np.linalg.norm(X, axis=1)
    floor = {"cosine": np.ones_like(xn), "inner_product": qn * xn, "l2": qn * qn + xn * xn}[metric]
    scale = np.maximum(np.abs(ref), floor + 1e-30)
    assert np.max(np.abs(fast - ref) / scale) < 1e-5


def _oracle_graph(orc, metric, n, dim, M, efc, order, seed=42, deletes=0):
    X = gauss(n, dim, seed)
    ids = (np.arange(n, dtype=np.int64) * 7 + 3)
    o = orc.Oracle(dim, metric, M, efc, order=order)
    assert o.insert_many(ids, X) == 0
    if deletes:
        rng = np.random.default_rng(seed + 1)
        for d in ids[rng.choice(n, deletes, replace=False)]:
            o.delete(int(d))
    return o, ids, X


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("order", ["sse", "wave"])
@pytest.mark.parametrize("shape", [(2000, 32, 16, 200), (600, 128, 16, 100), (400, 7, 4, 30), (300, 768, 8, 40)])
def test_search_over_fixed_graph_bit_exact(gpu, orc, metric, order, shape):
    n, dim, M, efc = shape
    oo = orc.ORDER_SSE if order == "sse" else orc.ORDER_WAVE
    go = gpu.ORDER_SSE if order == "sse" else gpu.ORDER_WAVE
    o, ids, X = _oracle_graph(orc, metric, n, dim, M, efc, oo, deletes=n // 20)
    g = gpu.HnswIndex(dim, metric, M, efc, order=go)
    g.load_graph_from(o, ids, X)
    assert g.node_count == o.node_count
    Q = gauss(64, dim, 99)
    for k, ef in ((1, 1), (10, 10), (10, 20), (10, 64), (10, 128), (50, 300)):
        wi, wd, wc = o.search_many(Q, k, ef)
        gi, gd, gc = g.search_batch(Q, k, ef)
        assert np.array_equal(gc, wc), (k, ef)
        assert np.array_equal(gi, wi), (k, ef)
        assert same_bits(gd, wd), (k, ef)
    # single-query entry point (hnsw_search) agrees with the batch
    i1, d1 = g.search(Q[0], 10, 64)
    wi, wd = o.search(Q[0], 10, 64)
    assert np.array_equal(i1, wi) and same_bits(d1, wd)
    g.close()


def test_search_with_duplicate_vectors_ties(gpu, orc):
    """Equal distances: pop order among ties is decided by the heap's sift rules
    (src/priority_queue.c:18-42); the device heaps must reproduce it."""
    dim, n = 16, 600
    base = gauss(60, dim, 5)
    X = base[np.random.default_rng(6).integers(0, 60, n)]  # many exact duplicates
    ids = np.arange(1, n + 1, dtype=np.int64)
    for metric in METRICS:
        o = orc.Oracle(dim, metric, 8, 60)
        o.insert_many(ids, X)
        g = gpu.HnswIndex(dim, metric, 8, 60)
        g.load_graph_from(o, ids, X)
        Q = base[:32] + 0.0
        for ef in (10, 40, 100):
            wi, wd, wc = o.search_many(Q, 10, ef)
            gi, gd, gc = g.search_batch(Q, 10, ef)
            assert np.array_equal(gi, wi), (metric, ef)
            assert same_bits(gd, wd)
        g.close()


def test_empty_and_tiny_index(gpu, orc):
    g = gpu.HnswIndex(4, "l2", 4, 10)
    ids, ds = g.search(np.zeros(4, np.float32), 5, 10)
    assert len(ids) == 0  # src/hnsw_algo.c:671
    assert g.insert(42, np.array([1, 2, 3, 4], np.float32)) == 0
    assert g.insert(42, np.array([1, 2, 3, 4], np.float32)) == -1  # duplicate (:522)
    assert g.entry_point == 42 and g.node_count == 1
    assert np.array_equal(g.get_vector(42), np.array([1, 2, 3, 4], np.float32))
    ids, ds = g.search(np.array([1, 2, 3, 5], np.float32), 3, 10)
    assert ids.tolist() == [42] and ds[0] == np.float32(1.0)
    g.close()


@pytest.mark.parametrize("metric", ["l2", "cosine"])
@pytest.mark.parametrize("order", ["sse", "wave"])
def test_batched_build_matches_oracle_schedule(gpu, orc, metric, order):
    """Batch-synchronous build: identical graph to the CPU restatement of the same schedule."""
    n, dim, M, efc = 3000, 24, 8, 60
    oo = orc.ORDER_SSE if order == "sse" else orc.ORDER_WAVE
    go = gpu.ORDER_SSE if order == "sse" else gpu.ORDER_WAVE
    X = gauss(n, dim, 11)
    ids = np.arange(100, 100 + n, dtype=np.int64)
    o = orc.Oracle(dim, metric, M, efc, order=oo)
    g = gpu.HnswIndex(dim, metric, M, efc, order=go)
    pos = 0
    for b in (1, 1, 1, 5, 20, 100, 372, 1000, 1500):
        assert o.insert_batch(ids[pos:pos + b], X[pos:pos + b]) == 0
        assert g.insert_batch(ids[pos:pos + b], X[pos:pos + b], gpu.BUILD_BATCHED) == 0
        pos += b
    assert pos == n
    assert g.graph(ids) == o.graph(ids)
    Q = gauss(50, dim, 12)
    wi, wd, wc = o.search_many(Q, 10, 64)
    gi, gd, gc = g.search_batch(Q, 10, 64)
    assert np.array_equal(gi, wi) and same_bits(gd, wd)
    g.close()


def test_batched_build_with_ties_matches_oracle(gpu, orc):
    """Duplicate vectors force distance ties inside the MN-RU prune (src/hnsw_algo.c:620-639)."""
    dim, n = 8, 1200
    base = gauss(40, dim, 21)
    X = base[np.random.default_rng(22).integers(0, 40, n)]
    ids = np.arange(1, n + 1, dtype=np.int64)
    for metric in ("l2", "cosine"):
        o = orc.Oracle(dim, metric, 4, 40)
        g = gpu.HnswIndex(dim, metric, 4, 40)
        pos = 0
        for b in (1, 3, 16, 80, 300, 800):
            o.insert_batch(ids[pos:pos + b], X[pos:pos + b])
            assert g.insert_batch(ids[pos:pos + b], X[pos:pos + b], gpu.BUILD_BATCHED) == 0
            pos += b
        assert g.graph(ids) == o.graph(ids), metric
        g.close()


def test_delete_matches_oracle(gpu, orc):
    n, dim = 800, 16
    X = gauss(n, dim, 31)
    ids = np.arange(1, n + 1, dtype=np.int64)
    o = orc.Oracle(dim, "l2", 8, 50)
    o.insert_many(ids, X)
    g = gpu.HnswIndex(dim, "l2", 8, 50)
    g.load_graph_from(o, ids, X)
    rng = np.random.default_rng(32)
    dels = [int(o.entry_point)] + [int(x) for x in ids[rng.choice(n, 60, replace=False)]]
    for d in dels:
        ro = o.delete(d)
        rg = g.delete(d)
        assert ro == rg
    assert g.delete(dels[0]) == -1  # already deleted
    assert g.graph(ids) == o.graph(ids)
    assert g.node_count == o.node_count and g.entry_point == o.entry_point
    Q = gauss(40, dim, 33)
    wi, wd, wc = o.search_many(Q, 10, 64)
    gi, gd, gc = g.search_batch(Q, 10, 64)
    assert np.array_equal(gi, wi) and same_bits(gd, wd)
    g.close()


@pytest.mark.parametrize("tag", ["a", "b", "c", "d", "e"])
def test_search_matches_reference_golden(gpu, tag):
    """The graph the COMPILED REFERENCE built (tests/golden/hnsw_*.npz) is loaded into HBM and searched
    by the HIP kernel: ids and f32 distance bits must equal what the reference itself returned."""
    import os

    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", f"hnsw_{tag}.npz"))
    n, d, M, efc, metric = int(z["n"]), int(z["dim"]), int(z["M"]), int(z["efc"]), str(z["metric"])
    X = gauss(n, d, int(z["seed_x"]))
    Q = gauss(200, d, int(z["seed_q"]))
    g = gpu.HnswIndex(d, metric, M, efc)  # default order = MN_ORDER_SSE = the reference's
    for i in range(n):
        assert g.load_node(i + 1, X[i], int(z["levels"][i])) == 0
    for row in z["rows"]:
        nb = row[2:][row[2:] >= 0]
        assert g.load_neighbors(int(row[0]), int(row[1]), nb.copy()) == 0
    g.set_entry(int(z["entry"]), int(z["max_level"]))
    for ef in (20, 64, 128, 256):
        gi, gd, gc = g.search_batch(Q, 10, ef)
        assert np.array_equal(gi, z[f"ids_ef{ef}"]), (tag, ef)
        assert np.array_equal(gd.view(np.int32), z[f"dist_ef{ef}"]), (tag, ef)
        assert np.array_equal(gc, z[f"cnt_ef{ef}"])
    # delete the same nodes the reference deleted; graph surgery + new entry point + search must agree
    for x in z["dels"]:  # the reference accepted every one of these: so must the device (lists grow as its lists grow)
        assert g.delete(int(x)) == 0, (tag, int(x), gpu.hnsw._err())
    assert g.entry_point == int(z["entry_after_delete"]) and g.node_count == int(z["node_count_after_delete"])
    gi, gd, gc = g.search_batch(Q, 10, 64)
    assert np.array_equal(gi, z["ids_after_delete"]) and np.array_equal(gd.view(np.int32), z["dist_after_delete"])
    g.close()


def test_full_size_properties(gpu):
    """Size-independent properties at a size the oracle would not finish quickly: every returned list
    is ascending, ids are valid and distinct, a stored vector finds itself at distance ~0, and search
    is idempotent."""
    n, d = 200_000, 96
    X = gauss(n, d, 77)
    ids = np.arange(1, n + 1, dtype=np.int64)
    g = gpu.HnswIndex(d, "l2", 16, 100, order=gpu.ORDER_WAVE)
    assert g.build(ids, X) == 0
    assert g.node_count == n
    Q = X[:2000] + 0.0
    i1, d1, c1 = g.search_batch(Q, 10, 64)
    i2, d2, c2 = g.search_batch(Q, 10, 64)
    assert np.array_equal(i1, i2) and same_bits(d1, d2)
    assert (c1 == 10).all()
    assert (np.diff(d1, axis=1) >= 0).all()
    assert ((i1 >= 1) & (i1 <= n)).all()
    assert all(len(set(r.tolist())) == 10 for r in i1)
    # a stored vector that finds itself does so at distance exactly 0 and in first place; widening the
    # beam never loses hits (recall on isotropic Gaussian data is low by the reference's own algorithm)
    hit64 = i1[:, 0] == ids[:2000]
    assert hit64.any() and np.all(d1[hit64, 0] == 0.0) and np.all(d1 >= 0.0)
    i3, d3, c3 = g.search_batch(Q, 10, 400)
    assert np.mean(i3[:, 0] == ids[:2000]) >= np.mean(hit64)
    assert np.mean(d3[:, 9]) <= np.mean(d1[:, 9])
    g.close()


def _golden_rows(g, ids, width):
    rows = []
    for i in ids:
        for l in range(g.node_level(int(i)) + 1):
            nb = g.neighbors(int(i), l)
            row = np.full(width + 2, -1, np.int64)
            row[0], row[1] = i, l
            row[2:2 + len(nb)] = nb
            rows.append(row)
    return np.array(rows, np.int64)


@pytest.mark.parametrize("tag", ["a", "b", "c", "d", "e"])
def test_sequential_insert_reproduces_reference_graph(gpu, tag):
    """hnsw_insert semantics on the device (k_insert_seq): levels, every neighbour list in order, entry
    point and max level equal what the compiled reference built from the same vectors."""
    import os

    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", f"hnsw_{tag}.npz"))
    n, d, M, efc, metric = int(z["n"]), int(z["dim"]), int(z["M"]), int(z["efc"]), str(z["metric"])
    X = gauss(n, d, int(z["seed_x"]))
    ids = np.arange(1, n + 1, dtype=np.int64)
    g = gpu.HnswIndex(d, metric, M, efc)
    # mix of the single-insert entry point and the multi-insert call
    for i in range(5):
        assert g.insert(int(ids[i]), X[i]) == 0
    assert g.insert_batch(ids[5:], X[5:], gpu.BUILD_SEQUENTIAL) == 0
    assert np.array_equal(np.array([g.node_level(int(i)) for i in ids], np.int8), z["levels"])
    assert np.array_equal(_golden_rows(g, ids, 2 * M), z["rows"])
    assert g.entry_point == int(z["entry"]) and g.max_level == int(z["max_level"])
    g.close()


def test_sequential_insert_with_ties_matches_oracle(gpu, orc):
    dim, n = 8, 900
    base = gauss(30, dim, 41)
    X = base[np.random.default_rng(42).integers(0, 30, n)]
    ids = np.arange(1, n + 1, dtype=np.int64)
    for metric in ("l2", "cosine", "inner_product"):
        o = orc.Oracle(dim, metric, 4, 40)
        o.insert_many(ids, X)
        g = gpu.HnswIndex(dim, metric, 4, 40)
        assert g.insert_batch(ids, X, gpu.BUILD_SEQUENTIAL) == 0
        assert g.graph(ids) == o.graph(ids), metric
        g.close()


@pytest.mark.parametrize("M,n,efc,dups", [(32, 1000, 100, False), (32, 400, 100, True), (48, 200, 110, True),
                                          (64, 200, 140, False)])  # exact inserts of wide rows are slow (one wavefront, ≤ 128 prunes each)
def test_wide_rows(gpu, orc, dups, M, n, efc):
    """M=32: a level-0 row is 64 links = one wavefront and the MN-RU prune sees 65 entries.  M=48 / 64: rows of 96 / 128
    links are walked in two 64-link passes everywhere (search, link, prune with up to 129 entries, persistence)."""
    dim = 12
    X = gauss(n, dim, 51)
    if dups:
        X = X[np.random.default_rng(52).integers(0, 90, n)]
    ids = np.arange(1, n + 1, dtype=np.int64)
    Q = gauss(40, dim, 53)
    for metric in ("l2", "cosine"):
        o = orc.Oracle(dim, metric, M, efc)
        o.insert_many(ids, X)
        g = gpu.HnswIndex(dim, metric, M, efc)
        assert g.insert_batch(ids, X, gpu.BUILD_SEQUENTIAL) == 0
        assert g.graph(ids) == o.graph(ids), metric
        assert max(len(v) for (_, l), v in o.graph(ids)["nbrs"].items() if l == 0) == 2 * M  # rows did fill
        wi, wd, wc = o.search_many(Q, 10, 80)
        gi, gd, gc = g.search_batch(Q, 10, 80)
        assert np.array_equal(gi, wi) and same_bits(gd, wd)
        g.close()
        ob = orc.Oracle(dim, metric, M, efc)
        gb = gpu.HnswIndex(dim, metric, M, efc)
        pos = 0
        for b in (1, 2, 7, 40, n - 50):
            assert ob.insert_batch(ids[pos:pos + b], X[pos:pos + b]) == 0
            assert gb.insert_batch(ids[pos:pos + b], X[pos:pos + b], gpu.BUILD_BATCHED) == 0
            pos += b
        assert pos == n
        assert gb.graph(ids) == ob.graph(ids), metric
        for d in [int(x) for x in ids[::37]]:
            assert gb.delete(d) == ob.delete(d) == 0, (d, gpu.hnsw._err())
        assert gb.graph(ids) == ob.graph(ids), metric
        gb.close()


def test_reference_binary_searches_device_built_graph(gpu, orc):
    """bench.py's cpu_baseline kind "reference": a GPU-built graph loaded into the compiled reference through the
    reference's own load API gives the same graph and bit-identical search results (SSE order)."""
    if not orc.have_ref():
        pytest.skip("oracle/_ref not built (needs /root/reference at build time)")
    n, dim, M, efc = 3000, 24, 8, 60
    X = gauss(n, dim, 61)
    ids = np.arange(10, 10 + n, dtype=np.int64)
    g = gpu.HnswIndex(dim, "cosine", M, efc)
    assert g.insert_batch(ids, X, gpu.BUILD_BATCHED) == 0
    for d in (17, 300, 2999):
        assert g.delete(d) == 0
    r = orc.Ref(dim, "cosine", M, efc)
    r.load_from_device(g, vectors=X)
    assert r.graph(ids)["nbrs"] == g.graph(ids)["nbrs"]
    Q = gauss(64, dim, 62)
    ri, rd, rc = r.search_many(Q, 10, 64)
    gi, gd, gc = g.search_batch(Q, 10, 64)
    assert np.array_equal(gi, ri) and same_bits(gd, rd)
    g.close()


def test_speculative_exact_inserts_equal_the_single_wavefront_kernel(gpu, monkeypatch):
    """mn_spec.hip: windows of inserts searched at once and committed in order up to the first stale one must leave
    the graph k_insert_seq leaves (which the golden tests pin to the reference) — on an index large enough for windows
    to commit several inserts, with duplicates so that the tie path of the parallel commit is exercised."""
    n0, n1, dim, M, efc = 30000, 1500, 16, 8, 60
    X = gauss(n0 + n1, dim, 71)
    X[n0 + 100:n0 + 400] = X[np.random.default_rng(72).integers(0, n0, 300)]  # exact duplicates of indexed vectors
    ids = np.arange(1, n0 + n1 + 1, dtype=np.int64)
    graphs = []
    for spec in ("0", "1"):
        monkeypatch.setenv("MN_SPECULATE", spec)
        g = gpu.HnswIndex(dim, "l2", M, efc)
        assert g.build(ids[:n0], X[:n0], 16, 4096) == 0
        assert g.insert_batch(ids[n0:], X[n0:], gpu.BUILD_SEQUENTIAL) == 0
        graphs.append((g.export_links(0), g.export_links(1), g.entry_point, g.max_level))
        g.close()
    assert np.array_equal(graphs[0][0], graphs[1][0]) and np.array_equal(graphs[0][1], graphs[1][1])
    assert graphs[0][2:] == graphs[1][2:]


@pytest.mark.parametrize("metric,dim", [("l2", 24), ("cosine", 40)])
def test_speculative_windows_with_colliding_inserts_equal_the_single_wavefront_kernel(gpu, monkeypatch, metric, dim):
    """Round 4: a window's insert stays valid when the rows its search read were rewritten in ways that cannot have changed the
    search (mn_spec.hip spec_rewrite_is_harmless).  The dangerous cases are rewrites that DO matter: consecutive inserts that
    are each other's nearest neighbours (the node an earlier insert appended to a row is one the later search would have
    pushed), runs from one small cluster (pruned rows drop neighbours the later search did push), exact duplicates (ties:
    the log's defaults), a small index (every window collides) and deleted nodes in the lists.  Same graph as the
    one-wavefront kernel, links, levels, entry point — with the windows on and off."""
    rng = np.random.default_rng(171)
    n0, M, efc = 4000, 8, 80
    centres = rng.standard_normal((12, dim)).astype(np.float32) * 3
    base = (centres[rng.integers(0, 12, n0)] + rng.standard_normal((n0, dim)).astype(np.float32) * 0.3).astype(np.float32)
    chain = np.cumsum(rng.standard_normal((400, dim)).astype(np.float32) * 0.01, axis=0) + centres[3]   # each next to the last
    burst = (centres[5] + rng.standard_normal((400, dim)).astype(np.float32) * 0.05).astype(np.float32)  # one tight cluster
    dups = base[rng.integers(0, n0, 200)]                                                                # ties
    far = rng.standard_normal((400, dim)).astype(np.float32) * 3                                         # harmless collisions
    new = np.concatenate([chain, far, burst, dups, chain[::-1] + np.float32(0.001), far[:100] * np.float32(1.001)]).astype(np.float32)
    X = np.concatenate([base, new])
    ids = np.arange(1, len(X) + 1, dtype=np.int64)
    graphs = []
    for spec in ("0", "1"):
        monkeypatch.setenv("MN_SPECULATE", spec)
        g = gpu.HnswIndex(dim, metric, M, efc)
        assert g.build(ids[:n0], X[:n0], 16, 1024) == 0
        for i in range(100, 160):  # deleted nodes stay in their neighbours' lists
            assert g.delete(int(ids[i])) == 0
        assert g.insert_batch(ids[n0:], X[n0:], gpu.BUILD_SEQUENTIAL) == 0
        graphs.append((g.export_links(0), g.export_links(1), g.export_nodes()[1], g.entry_point, g.max_level))
        g.close()
    for a, b in zip(graphs[0][:3], graphs[1][:3]):
        assert np.array_equal(a, b)
    assert graphs[0][3:] == graphs[1][3:]


@pytest.mark.parametrize("seed", [1, 2, 3, 4, 5, 6])
def test_speculative_windows_random_configurations_equal_the_single_wavefront_kernel(gpu, monkeypatch, seed):
    """The window rules of mn_spec.hip on random small configurations where they bite hardest: small ef_construction (the
    results are full after a few rows, so the "could have been pushed" masks and bounds decide, not the +inf of a filling queue),
    small M (every row is full: every link is a prune that reorders the list), few dimensions and coarse coordinates (equal
    distances: the heaps' searches and their order rule), clusters, several upper layers (greedy steps over rewritten rows)."""
    rng = np.random.default_rng(1000 + seed)
    dim = int(rng.integers(2, 12))
    M = int(rng.choice([2, 3, 4, 6, 8]))
    efc = int(rng.choice([4, 8, 16, 40]))
    metric = ["l2", "cosine", "inner_product"][seed % 3]
    n0, n1 = int(rng.integers(600, 3000)), 1200
    k = int(rng.integers(3, 40))
    centres = rng.standard_normal((k, dim)) * 2
    X = centres[rng.integers(0, k, n0 + n1)] + rng.standard_normal((n0 + n1, dim)) * rng.choice([0.05, 0.3, 1.0])
    if seed % 2 == 0:
        X = np.round(X * 4) / 4  # coarse coordinates: many equal distances
    X = X.astype(np.float32)
    if metric != "l2":
        X[np.abs(X).sum(1) == 0] += 1.0
    ids = np.arange(1, n0 + n1 + 1, dtype=np.int64)
    graphs = []
    for spec in ("0", "1"):
        monkeypatch.setenv("MN_SPECULATE", spec)
        g = gpu.HnswIndex(dim, metric, M, efc)
        assert g.insert_batch(ids[:n0], X[:n0], gpu.BUILD_SEQUENTIAL) == 0
        for i in range(50, 50 + n0 // 20):
            assert g.delete(int(ids[i])) == 0
        assert g.insert_batch(ids[n0:], X[n0:], gpu.BUILD_SEQUENTIAL) == 0
        lv = g.export_nodes()[1]
        graphs.append(([g.export_links(l) for l in range(int(lv.max()) + 1)], lv, g.entry_point, g.max_level))
        g.close()
    assert graphs[0][2:] == graphs[1][2:] and np.array_equal(graphs[0][1], graphs[1][1])
    assert len(graphs[0][0]) == len(graphs[1][0])
    for a, b in zip(graphs[0][0], graphs[1][0]):
        assert np.array_equal(a, b)


def test_two_host_threads_two_indexes(gpu, orc):
    """SURVEY §8b threading contract: one host thread per connection, several connections per process.  Each index has
    its own HIP stream and the device is selected per call; two threads building and searching their own indexes at
    the same time must get what they get alone (ctypes releases the GIL during the calls)."""
    import threading

    dim, n = 16, 2500
    data = [(gauss(n, dim, 81 + t), gauss(40, dim, 91 + t)) for t in range(2)]
    ids = np.arange(1, n + 1, dtype=np.int64)
    want = []
    for X, Q in data:
        o = orc.Oracle(dim, "l2", 8, 60)
        o.insert_many(ids, X)
        want.append(o.search_many(Q, 5, 40))
    got, errs = [None, None], []

    def work(t):
        try:
            X, Q = data[t]
            g = gpu.HnswIndex(dim, "l2", 8, 60)
            for a in range(0, n, 500):  # exact inserts, several launches, interleaved with the other thread's
                assert g.insert_batch(ids[a:a + 500], X[a:a + 500], gpu.BUILD_SEQUENTIAL) == 0
                g.search_batch(Q, 5, 40)
            got[t] = g.search_batch(Q, 5, 40)
            g.close()
        except Exception as e:  # noqa: BLE001
            errs.append(e)

    th = [threading.Thread(target=work, args=(t,)) for t in range(2)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errs, errs
    for t in range(2):
        assert np.array_equal(got[t][0], want[t][0]) and same_bits(got[t][1], want[t][1])


def test_rowid_minus_one_is_also_the_empty_marker(gpu, orc):
    """-1 is a legal rowid and the reference's "no entry point" value (src/hnsw_algo.c:194,:544): after rowid -1 goes
    into an empty index the next insert is treated as the first one again.  Same here, in one call or several."""
    X = gauss(6, 4, 95)
    ids = np.array([-1, 14, 3, -7, 0, 9], np.int64)
    o = orc.Oracle(4, "l2", 4, 20)
    o.insert_many(ids, X)
    for cuts in ([6], [1, 5], [2, 4]):
        g = gpu.HnswIndex(4, "l2", 4, 20)
        a = 0
        for b in cuts + [6]:
            if b > a:
                assert g.insert_batch(ids[a:b], X[a:b], gpu.BUILD_SEQUENTIAL) == 0
            a = b
        assert g.graph(ids) == o.graph(ids), cuts
        assert g.entry_point == o.entry_point and g.max_level == o.max_level
        g.close()


def test_m_beyond_the_lds_budget_is_refused_loudly(gpu):
    gpu.HnswIndex(8, "l2", 65, 50).close()  # (refused in round 1; rows are no longer fixed-width)
    with pytest.raises(Exception):
        gpu.HnswIndex(8, "l2", 513, 50)


def test_baseline_full_size_1Mx768(gpu, orc):
    """BASELINE.json configs[1] at full size: 1M x 768 f32 cosine, M=16, efC=200, 10k queries, k=10, ef=128.
    Size-independent properties (ascending, valid, distinct, idempotent, counters consistent) plus a direct
    comparison of a query sample with the CPU oracle running on the SAME graph (bulk-exported)."""
    n, d, nq, k, ef = 1_000_000, 768, 10_000, 10, 128
    rng = np.random.default_rng(42)
    X = np.empty((n, d), np.float32)
    for a in range(0, n, 65536):
        X[a:a + 65536] = rng.standard_normal((min(65536, n - a), d), dtype=np.float32)
    ids = np.arange(1, n + 1, dtype=np.int64)
    Q = np.random.default_rng(43).standard_normal((nq, d), dtype=np.float32)
    g = gpu.HnswIndex(d, "cosine", 16, 200)
    assert g.build(ids, X) == 0 and g.node_count == n
    i1, d1, c1 = g.search_batch(Q, k, ef)
    st = g.last_launch()
    assert st["last_n_overflow"] == 0 and st["last_n_dist"] > nq * ef
    i2, d2, c2 = g.search_batch(Q, k, ef)
    assert np.array_equal(i1, i2) and same_bits(d1, d2)
    assert (c1 == k).all() and (np.diff(d1, axis=1) >= 0).all() and ((i1 >= 1) & (i1 <= n)).all()
    assert all(len(set(r.tolist())) == k for r in i1[:2000])
    lv = g.export_nodes()[1]
    assert lv.max() == g.max_level and 0.9 < (lv > 0).mean() * 16 < 1.1  # P(level >= 1) = 1/M
    rows = g.export_links(0)
    deg = (rows >= 0).sum(1)
    assert deg.max() <= 32 and deg.min() >= 1
    o = orc.Oracle(d, "cosine", 16, 200)
    o.load_from_device(g, vectors=X)
    wi, wd, wc = o.search_many(Q[:60], k, ef)
    assert np.array_equal(i1[:60], wi) and same_bits(d1[:60], wd)
    g.close()


# ───────────── lists longer than M_max, M > 64, a full node table: the reference has no fixed row width ─────────────

def _dev_index(gpu, mode):
    class Dev(gpu.HnswIndex):
        def insert_many(self, ids, vecs):
            return self.insert_batch(ids, vecs, mode)
    return Dev


@pytest.mark.gpu
def test_overgrown_lists_follow_the_reference(gpu, orc):
    """Deletes whose reconnection grows lists past M_max (src/hnsw_algo.c:775-782 over :142-163) and a loaded graph with
    lists of up to 3x M_max: the device rows grow as the reference's lists do (re-strided table, 64-link passes), searches
    walk the whole list, and later inserts prune such lists back to M_max (:601-646) — graph, ids and distance bits
    equal to the oracle, which tests/test_oracle_vs_ref.py pins to the compiled reference on this very case."""
    from util import overgrown_case

    o, ids, X, go = overgrown_case(orc.Oracle)
    g, _, _, gg = overgrown_case(_dev_index(gpu, gpu.BUILD_SEQUENTIAL))
    assert gg == go  # after the deletes, before the long lists were loaded
    assert max(len(v) for (_, l), v in go["nbrs"].items() if l == 0) > 4
    assert g.graph(ids[:1000]) == o.graph(ids[:1000])
    assert g.L.mn_hnsw_row_width(g.h, 0) > 4 and g.L.mn_hnsw_row_width(g.h, 1) > 2
    Q = gauss(30, 2, 77)
    wi, wd, _ = o.search_many(Q, 5, 20)
    gi, gd, _ = g.search_batch(Q, 5, 20)
    assert np.array_equal(gi, wi) and same_bits(gd, wd)
    assert g.insert_many(ids[1000:1150], X[1000:1150]) == 0 and o.insert_many(ids[1000:1150], X[1000:1150]) == 0
    assert g.graph(ids[:1150]) == o.graph(ids[:1150])  # exact inserts pruned the long lists they touched
    assert g.insert_batch(ids[1150:], X[1150:], gpu.BUILD_BATCHED) == 0 and o.insert_batch(ids[1150:], X[1150:]) == 0
    assert g.graph(ids) == o.graph(ids)  # so does the batch link step
    for v in ids[1000::3]:
        assert g.delete(int(v)) == o.delete(int(v)) == 0
    assert g.graph(ids) == o.graph(ids)
    wi, wd, _ = o.search_many(Q, 5, 20)
    gi, gd, _ = g.search_batch(Q, 5, 20)
    assert np.array_equal(gi, wi) and same_bits(gd, wd)
    g.close()


@pytest.mark.gpu
@pytest.mark.parametrize("M", [80, 130])
def test_m_above_64(gpu, orc, M):
    """The reference accepts any m >= 2 (src/hnsw_vtab.c:80-134): rows of 2M > 128 links, prune over 2M + 1 entries."""
    n, dim, efc = 700, 6, 150
    X = gauss(n, dim, 8)
    ids = np.arange(1, n + 1, dtype=np.int64)
    Q = gauss(25, dim, 9)
    o = orc.Oracle(dim, "cosine", M, efc)
    g = gpu.HnswIndex(dim, "cosine", M, efc)
    assert o.insert_many(ids[:450], X[:450]) == 0 and g.insert_batch(ids[:450], X[:450], gpu.BUILD_SEQUENTIAL) == 0
    assert g.graph(ids[:450]) == o.graph(ids[:450])
    assert max(len(v) for (_, l), v in o.graph(ids[:450])["nbrs"].items() if l == 0) == 2 * M  # rows did fill
    assert o.insert_batch(ids[450:], X[450:]) == 0 and g.insert_batch(ids[450:], X[450:], gpu.BUILD_BATCHED) == 0
    assert g.graph(ids) == o.graph(ids)
    for k, ef in ((10, 40), (30, 200)):
        wi, wd, _ = o.search_many(Q, k, ef)
        gi, gd, _ = g.search_batch(Q, k, ef)
        assert np.array_equal(gi, wi) and same_bits(gd, wd)
    for v in ids[::29]:
        assert g.delete(int(v)) == o.delete(int(v)) == 0
    assert g.graph(ids) == o.graph(ids)
    g.close()


@pytest.mark.gpu
def test_node_table_fills_under_churn_as_in_the_reference(gpu, orc):
    """insert 150, delete 150, insert 250: the reference's table (256 entries, grown on the live count only) fills and
    hnsw_insert fails from then on (src/hnsw_algo.c:61-74, :527-540) — same return codes, same surviving graph, the index
    stays usable (no out-of-bounds slot)."""
    d = 4
    X = gauss(400, d, 5)
    o = orc.Oracle(d, "l2", 4, 20)
    g = gpu.HnswIndex(d, "l2", 4, 20)
    ro, rg = [], []
    for i in range(150):
        ro.append(o.insert(i + 1, X[i])); rg.append(g.insert(i + 1, X[i]))
    for i in range(150):
        ro.append(o.delete(i + 1)); rg.append(g.delete(i + 1))
    for i in range(150, 400):
        ro.append(o.insert(i + 1, X[i])); rg.append(g.insert(i + 1, X[i]))
    assert rg == ro and -1 in ro[300:]
    live = [i + 1 for i in range(150, 400) if ro[150 + i] == 0]
    assert g.graph(live) == o.graph(live) and g.node_count == o.node_count
    wi, wd, _ = o.search_many(X[:20], 5, 30)
    gi, gd, _ = g.search_batch(X[:20], 5, 30)
    assert np.array_equal(gi, wi) and same_bits(gd, wd)
    # a batch that would hit the full table inserts nothing
    assert g.insert_batch(np.arange(1000, 1010, dtype=np.int64), X[:10], gpu.BUILD_BATCHED) == -1
    assert g.node_count == o.node_count and g.slot_count == 256
    g.close()


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("n,dim,nq,k", [(5000, 50, 300, 10), (1111, 7, 5, 1), (20000, 768, 130, 16)])
def test_mfma_bruteforce_ground_truth(gpu, metric, n, dim, nq, k, monkeypatch):
    """k_brute_mfma (the dense query x row block on the f32 matrix cores + fused top-k) and the VALU kernel that uses the
    index's own inner loop, each against float64 numpy: every returned row within rounding (a per-pair bound from the f32
    operation count) of the k-th distance, every row clearly nearer returned, the list ordered up to rounding
    (util.check_topk_f64)."""
    X = gauss(n, dim, 21)
    X[17] = X[3]  # exact duplicate rows: ties resolve to the lower row
    Q = gauss(nq, dim, 22)
    Q[0] = X[3]
    ids = np.arange(100, 100 + n, dtype=np.int64)
    g = gpu.HnswIndex(dim, metric, 8, 40)
    assert g.insert_batch(ids, X, gpu.BUILD_BATCHED) == 0
    for dl in (105, 140):
        assert g.delete(dl) == 0  # deleted rows never appear
    dq = g.dev_malloc(Q.nbytes)
    g.dev_upload(dq, Q)
    got = g.bruteforce_topk(dq, nq, k)
    monkeypatch.setenv("MN_BRUTE", "valu")
    valu = g.bruteforce_topk(dq, nq, k)
    monkeypatch.delenv("MN_BRUTE")
    assert not np.isin(got, [105, 140]).any() and (got >= 100).all()
    check_topk_f64(got, X, Q, ids, np.array([105, 140], np.int64), k, metric)
    check_topk_f64(valu, X, Q, ids, np.array([105, 140], np.int64), k, metric)
    assert got[0][0] in (103, 117) and (k == 1 or set(got[0][:2]) == {103, 117})  # the duplicated row, both copies
    g.dev_free(dq)
    g.close()


def test_batched_build_graph_is_as_good_as_the_exact_one(gpu):
    """The batch-synchronous build is what the headline index is built with; its graph differs from the reference's
    one-at-a-time graph.  Same vectors, both schedules: recall@10 (vs exact ground truth, all queries) within 0.01 at
    each ef, on embedding-like data and on the isotropic worst case.  (12k vectors here to keep the suite short; bench.py
    runs the same leg at 50k x 768 in every --full run and profiles/r02_graph_quality_100k.json holds 100k x 768 on three sets.)"""
    import argparse

    import bench

    args = argparse.Namespace(dim=64, nq=2000, k=10, metric="cosine")
    rows = bench.graph_quality_leg(gpu, args, 0, gpu.ORDER_SSE, 16, 200, 12_000, ["lowrank", "gaussian"], (64, 128))
    for r in rows:
        assert r["max_abs_recall_gap"] <= 0.01, r
    assert rows[0]["exact_recall_ef128"] > 0.9  # lowrank: the regime the recall target is quoted in


def test_wave_order_id_sets_against_the_reference_order_at_100k_x_768(gpu, orc):
    """MN_ORDER_WAVE (the fast summation order, ~1e-7 relative from the reference's) is checked bit for bit against its
    own CPU restatement elsewhere; here its RESULTS are held against the reference's order on the same graph at a size
    where near-ties could flip a neighbour: id-set mismatches are counted over 400 queries (north_star: bit-exact id sets,
    distances within 1e-5 relative)."""
    n, d, nq, k, ef = 100_000, 768, 400, 10, 128
    X = gauss(n, d, 91)
    Q = gauss(nq, d, 92)
    ids = np.arange(1, n + 1, dtype=np.int64)
    g = gpu.HnswIndex(d, "cosine", 16, 200, order=gpu.ORDER_WAVE)
    assert g.build(ids, X) == 0
    gi, gd, gc = g.search_batch(Q, k, ef)
    o = orc.Oracle(d, "cosine", 16, 200, order=orc.ORDER_SSE)  # the reference's summation order
    o.load_from_device(g, vectors=X)
    wi, wd, wc = o.search_many(Q, k, ef)
    mism = sum(set(gi[i].tolist()) != set(wi[i].tolist()) for i in range(nq))
    assert mism <= nq // 100, mism  # (measured: 0)
    same = [i for i in range(nq) if np.array_equal(gi[i], wi[i])]
    rel = np.abs(gd[same] - wd[same]) / np.maximum(np.abs(wd[same]), 1.0)
    assert rel.max() <= 1e-5
    g.close()


def test_bench_streamed_build_path(gpu):
    """bench.py's large-N path (the matrix is never held on the host: 10M x 768 is 30.7 GB) at a size that takes seconds."""
    import json
    import os
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--num-vectors", "150000", "--dim", "32", "--nq", "500",
                        "--stream-above", "50000", "--steps", "2", "--warmup", "1", "--dataset", "lowrank"],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-1500:]
    j = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert j["config"]["n"] == 150000 and j["recall_queries"] == 500 and j["recall_at_10"] > 0.8
    assert j["build_roofline"]["batches"] > 10 and j["cpu_baseline"] is None


def _bench(args, timeout=600):
    import json
    import os
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1"] + args, capture_output=True, text=True,
                       timeout=timeout)
    assert r.returncode == 0, r.stderr[-1500:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0])


def test_bench_plain_run_times_the_steps_and_dumps_the_last_step(gpu, tmp_path):
    """A plain run is set-up, warm-up, the timed steps and the line; --dump-outputs writes the last timed step's answers, and
    the same arguments give the same inputs, hence the same answers, in another process."""
    size = ["--num-vectors", "20000", "--dim", "64", "--nq", "500", "--steps", "3", "--warmup", "1"]
    runs = [_bench(size + ["--dump-outputs", str(tmp_path / t)]) for t in ("a", "b")]
    for j in runs:
        assert j["steps"] == 3 and j["warmup"] == 1 and j["ms_per_step"] > 0 and j["unit"] == "queries/s"
        assert abs(j["value"] - 500 / (j["ms_per_step"] * 1e-3)) <= 1e-6 * j["value"]
        assert j["recall_at_10"] is not None and j["roofline"]["kernel_ms"] > 0
        for leg in ("cpu_baseline", "parity_vs_oracle", "one_query_per_call", "wave_order", "at_recall_target",
                    "graph_quality_exact_vs_batched", "graph"):
            assert j[leg] is None, leg
        assert j["ef_sweep"] == []
    out = {}
    for t in ("a", "b"):
        out[t] = {n: np.load(tmp_path / t / f"{n}.npy") for n in ("neighbor_ids", "distances", "result_counts")}
    a = out["a"]
    assert a["neighbor_ids"].dtype == np.float64 and a["neighbor_ids"].shape == (500, 10)
    assert a["distances"].dtype == np.float32 and a["distances"].shape == (500, 10)
    assert a["result_counts"].dtype == np.float64 and (a["result_counts"] == 10).all()
    assert ((a["neighbor_ids"] >= 1) & (a["neighbor_ids"] <= 20000)).all()
    for n in a:
        assert same_bits(a[n], out["b"][n]), n


def test_bench_full_runs_the_other_legs(gpu, orc):
    """--full: everything beyond the headline (ef sweep, one query per call, CPU baseline and parity, wave-order, recall-target
    and graph-quality legs) at a size that takes seconds; the graph block has fixed sizes and is left out here."""
    j = _bench(["--full", "--num-vectors", "3000", "--dim", "32", "--nq", "200", "--steps", "2", "--warmup", "1",
                "--no-graph-block", "--quality-n", "1000", "--cpu-queries", "100", "--ref-queries", "50", "--exact-inserts", "50",
                "--target-datasets", "lowrank16"])
    assert j["steps"] == 2 and j["value"] > 0
    assert j["parity_vs_oracle"]["ids_identical"] and j["cpu_baseline"]["value"] > 0
    assert [r["ef"] for r in j["ef_sweep"]] == [128, 256, 512]
    assert j["one_query_per_call"]["queries"] == 200
    assert j["wave_order"] is not None and j["at_recall_target"]["datasets"][0]["dataset"] == "lowrank16"
    assert j["graph_quality_exact_vs_batched"][0]["n"] == 1000 and j["graph"] is None


def _bits(x):
    return int(np.float32(x).view(np.int32))


@pytest.mark.gpu
@pytest.mark.parametrize("metric,dim,m,deletes", [("cosine", 24, 4, False), ("l2", 7, 2, True), ("inner_product", 16, 8, True)])
def test_logged_insert_reports_exactly_the_edges_that_changed(gpu, metric, dim, m, deletes):
    """mn_hnsw_insert_logged: the same insert as mn_hnsw_insert plus the list of edges it added and removed (so that the
    extension rewrites ~100 "{t}_edges" rows per INSERT instead of ~1 100).  Two copies of one session: A persists edge by
    edge from the log and falls back to the persist set when there is none, B persists as the reference does — every node of
    the persist set rewritten whole (src/hnsw_vtab.c:755-776), deletes persisting nothing (:702-706).  After EVERY operation
    the two persisted edge sets (ids, levels, f32 distance bits) must be equal; and without deletes A's equals a full export.
    Small M: lists overflow and are pruned from the first few dozen rows; deletes leave edited lists un-persisted and dangling
    links whose distance a whole rewrite stores as 0 — the cases in which the log has to say "no log"."""
    n = 700
    rng = np.random.default_rng(12)
    X = rng.standard_normal((n, dim)).astype(np.float32)
    X[50] = X[10]  # duplicates: distance ties in the prunes (MN-RU looks at other rows)
    X[51] = X[10]
    ids = np.arange(100, 100 + n, dtype=np.int64)
    a = gpu.HnswIndex(dim, metric, m, 40)
    b = gpu.HnswIndex(dim, metric, m, 40)
    ea, eb = {}, {}

    def rewrite_whole(ix, store, nodes):
        nodes = set(int(x) for x in nodes)
        for k in [k for k in store if k[0] in nodes]:
            del store[k]
        if nodes:
            src, dst, lvl, dist = ix.edges_of(np.array(sorted(nodes), np.int64))
            for s_, d_, l_, x in zip(src, dst, lvl, dist):
                store[(int(s_), int(l_), int(d_))] = _bits(x)

    n_logged = n_unlogged = 0
    live = []
    for i in range(n):
        rc, log = a.insert_logged(ids[i], X[i])
        assert rc == 0 and b.insert(ids[i], X[i]) == 0
        rewrite_whole(b, eb, b.take_dirty())
        if log is None:
            n_unlogged += 1
            rewrite_whole(a, ea, a.take_dirty())
        else:
            n_logged += 1
            assert a.take_dirty().size == 0  # the log replaces the persist set
            for op, level, s_, d_, dist_ in log:
                if op == 1:
                    ea[(s_, level, d_)] = _bits(dist_)
                else:
                    assert (s_, level, d_) in ea, (i, s_, level, d_)
                    del ea[(s_, level, d_)]
        assert ea == eb, i
        live.append(int(ids[i]))
        if deletes and i > 30 and rng.random() < 0.15:
            d = live.pop(int(rng.integers(0, len(live))))
            assert a.delete(d) == 0 and b.delete(d) == 0
        if not deletes and (i % 97 == 0 or i == n - 1 or i < 40):
            full = {}
            rewrite_whole(a, full, ids[:i + 1])
            assert ea == full, i
    assert n_logged > n // 5, (n_logged, n_unlogged)
    assert (n_unlogged > 0) == deletes
    assert a.graph(ids) == b.graph(ids)
    # a rolled-back transaction: everything present is unknown until rewritten; new rows are logged again once they stop
    # touching unknown nodes
    a.log_invalidate()
    rc, log = a.insert_logged(10_000, X[0] * 0.5)
    assert rc == 0 and log is None and a.take_dirty().size > 0
    a.close()
    b.close()


@pytest.mark.gpu
@pytest.mark.parametrize("n,dim,metric", [(6000, 96, "l2"), (3000, 768, "cosine"), (2500, 300, "inner_product")])
def test_lone_search_kernel_equals_the_batch_kernel(gpu, n, dim, metric):
    """One query per launch runs in k_beam_coop with both queues in registers (unsorted arrays, cached nearest / worst, a tie or
    NaN sends the layer back to the binary heaps; rows of 256+ floats go through the per-wavefront LDS tile); a batch of more than
    128 queries runs in k_beam with the LDS heaps.  Same index, same queries: ids, distance bits and counts must be equal at
    every ef — below and above the 256 the registers hold, on data with exact duplicates (ties in both queues) as well."""
    rng = np.random.default_rng(77)
    X = rng.standard_normal((n, dim)).astype(np.float32)
    X[n // 2:n // 2 + 200] = X[:200]  # exact duplicates
    X[n - 50:] = 0.0                  # and a block of zero vectors (cosine: distance 1 for all of them)
    ids = np.arange(1, n + 1, dtype=np.int64)
    g = gpu.HnswIndex(dim, metric, 16, 100)
    assert g.build(ids, X) == 0
    Q = np.concatenate([rng.standard_normal((150, dim)).astype(np.float32), X[:30], np.zeros((2, dim), np.float32)])
    for ef in (10, 64, 200, 256, 300):
        bi, bd, bc = g.search_batch(Q, 10, ef)  # 182 queries: k_beam
        bst = g.last_launch()
        nd = nx = 0
        for qi in range(len(Q)):
            si, sd = g.search(Q[qi], 10, ef)    # one query: k_beam_coop
            assert len(si) == bc[qi], (ef, qi)
            assert np.array_equal(si, bi[qi, :bc[qi]]), (ef, qi)
            assert same_bits(sd, bd[qi, :bc[qi]]), (ef, qi)
            st = g.last_launch()                # (the lone path's counters come back in its pinned block, per query)
            assert st["last_n_overflow"] == 0
            nd += st["last_n_dist"]
            nx += st["last_n_expanded"]
        # the same searches: the same number of distances and expansions, whichever kernel and queue ran them
        assert (nd, nx) == (bst["last_n_dist"], bst["last_n_expanded"]), ef
    g.close()


_KNOB_SCRIPT = r"""
import os, sys
import numpy as np
sys.path.insert(0, os.environ["MN_ROOT"])
import muninn_amd
from oracle import orc
pkg = muninn_amd.pkg
rng = np.random.default_rng(5)
for dim, metric, n in ((768, "cosine", 420), (512, "l2", 400), (300, "l2", 500), (24, "inner_product", 700)):
    X = rng.standard_normal((n, dim)).astype(np.float32)
    X[100:110] = X[:10]  # ties
    ids = np.arange(1, n + 1, dtype=np.int64)
    o = orc.Oracle(dim, metric, 8, 60)
    o.insert_many(ids, X)
    g = pkg.HnswIndex(dim, metric, 8, 60)
    for i in range(n):  # one at a time: k_insert_seq
        assert g.insert(int(ids[i]), X[i]) == 0
    assert g.graph(ids) == o.graph(ids), (dim, metric)
    Q = rng.standard_normal((40, dim)).astype(np.float32)
    for q in Q:
        gi, gd = g.search(q, 10, 64)  # one at a time: k_beam_coop
        oi, od = o.search(q, 10, 64)
        assert np.array_equal(gi, oi) and np.array_equal(gd.view(np.int32), od.view(np.int32)), (dim, metric)
    g.close()
print("OK")
"""


@pytest.mark.gpu
@pytest.mark.parametrize("knob", ["MN_LDS_OPTIN", "MN_LAT_TILE", "MN_SEQ_PRE", "MN_COOP", "MN_SPECULATE"])
def test_latency_kernel_fallbacks_give_the_same_graph_and_answers(gpu, knob):
    """The lone-search / lone-insert kernels pick their LDS geometry at launch: a 4-row distance tile per wavefront when the device
    grants room for it (else 2 rows, else none), precomputed prune distances when they fit, helper wavefronts.  Every knob
    that switches one of these off (MN_LDS_OPTIN=0 takes 512-d to the 2-row tile; with the 160 KB opt-in of this part the 2-row
    tile is taken from about 950 floats and none above about 1500 — test_row_lengths.py asserts each) must leave the
    graph of one-at-a-time inserts and the answers of one-at-a-time queries equal to the oracle's, bit for bit (ids, distance
    bits), at dimensions that use the tile (768, 512, 300) and one that does not (24)."""
    import os
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, MN_ROOT=root)
    env[knob] = "0"
    r = subprocess.run([sys.executable, "-c", _KNOB_SCRIPT], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "OK" in r.stdout, r.stderr[-1500:]


@pytest.mark.parametrize("metric,M,dup", [("l2", 16, False), ("cosine", 8, True), ("inner_product", 16, False), ("l2", 40, True)])
def test_batched_link_step_with_hub_targets_equals_the_oracle(gpu, orc, metric, M, dup):
    """One batch whose thousands of nodes all link back to a few dozen existing nodes: every existing node is a hub that
    receives hundreds to thousands of reverse edges in ONE link step.  k_link_reverse scores such a target's sources 64 at a
    time and keeps the M_max nearest (round 4) instead of replaying thousands of prunes; the oracle replays them one by one
    (src/hnsw_algo.c:583-653).  Same rows, bit for bit — also when duplicate vectors tie (those targets go back to the
    reference's steps), on upper layers, and with the batch index order scrambled by the hash of the bins."""
    dim, n0, nb = 12, 70, 3000
    X = gauss(n0 + nb, dim, 77)
    if dup:
        X[n0 + 5:n0 + nb:37] = X[n0 + 5]      # many copies of one batch vector: equal distances to every target
        X[n0 + 9:n0 + nb:101] = X[3]          # and copies of an existing node
    ids = np.arange(1, n0 + nb + 1, dtype=np.int64)
    o = orc.Oracle(dim, metric, M, 60)
    g = gpu.HnswIndex(dim, metric, M, 60)
    for lo, hi in ((0, 1), (1, 8), (8, n0), (n0, n0 + nb)):
        assert o.insert_batch(ids[lo:hi], X[lo:hi]) == 0
        assert g.insert_batch(ids[lo:hi], X[lo:hi], gpu.BUILD_BATCHED) == 0
    assert g.graph(ids) == o.graph(ids)
    # and a second large batch on top of the grown graph (rows are full now: every append overflows)
    X2 = gauss(2500, dim, 78)
    ids2 = np.arange(10_001, 12_501, dtype=np.int64)
    assert o.insert_batch(ids2, X2) == 0
    assert g.insert_batch(ids2, X2, gpu.BUILD_BATCHED) == 0
    assert g.graph(np.concatenate([ids, ids2])) == o.graph(np.concatenate([ids, ids2]))
    g.close()
