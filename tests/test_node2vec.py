"""Node2Vec (src/node2vec.c): the oracle's serial restatement against the embedding bytes the compiled
reference produced through its own SQL function (tests/golden/node2vec.npz), and the HIP sequential
kernel against the same bytes.  Plus the reference's statistical acceptance tests
(pytests/test_node2vec.py:194-273)."""
import os

import numpy as np
import pytest

from oracle import orc_graph as og
from oracle.graph_cases import n2v_cases

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = n2v_cases()


def _graph(edges):
    e = np.array(edges, np.int32)
    return og.N2vGraph(e[:, 0], e[:, 1])


def _star(leaves):
    """a hub (first-seen index 0) and `leaves` leaves whose only neighbour is the hub"""
    return _graph([(0, i) for i in range(1, leaves + 1)])


def _dead_end_graph(n=203, seed=5):
    """n nodes of an undirected random graph (mean degree ~6) in which at least six nodes are isolated (walks of one
    node) and three are dead ends: their neighbours list them, they list nobody, so a walk that reaches one ends there,
    at any step.  Given as CSR (node i = index i): an edge table can express neither."""
    r = np.random.default_rng(seed)
    isolated, dead = {0, 9, 64, 65, 131, n - 1}, {17, 100, 150}
    lists = [[] for _ in range(n)]
    for a, b in r.integers(0, n, (3 * n, 2)).tolist():
        if a != b and a not in isolated and b not in isolated and b not in lists[a]:
            lists[a].append(b)
            lists[b].append(a)
    for d in dead:
        lists[d] = []
    off = np.concatenate([[0], np.cumsum([len(x) for x in lists])])
    return og.N2vGraph.from_csr(off, [x for lst in lists for x in lst])


def _n2v_template(dim):
    """n2v_for_width (csrc/mn_n2v_batched.hpp) → (NR register slots per lane, PF target rows in flight per chunk in
    k_n2v_walk_grad, U source rows in flight in k_n2v_apply)"""
    nr = (dim + 63) // 64
    NR = next(t for t in (1, 2, 4, 8, 16) if nr <= t)
    return NR, 6 if NR <= 4 else 2, 8 if NR <= 2 else 4 if NR <= 4 else 1


def _n2v_split(p, q, walk_length, walks):
    """wavefronts that share one walk in k_n2v_walk_grad (n2v_samples), for a batch of `walks` walks"""
    split = -(-32768 // walks) if p == 1.0 and q == 1.0 else 1
    return max(1, min(split, 8, walk_length))


def _seq_vs_oracle(gpu, g, prm):
    want, npairs = og.node2vec_train(g, *prm)
    got, st = gpu.node2vec_train(g.off, g.adj, *prm)
    assert st["pairs"] == npairs
    assert np.array_equal(got.view(np.int32), want.view(np.int32))
    return npairs


def _batched_vs_oracle(gpu, g, prm, batch):
    want, npairs = og.node2vec_train_batched(g, *prm, batch)
    got, st = gpu.node2vec_train(g.off, g.adj, *prm, mode=gpu.N2V_BATCHED, batch_walks=batch)
    assert st["pairs"] == npairs
    assert np.array_equal(got.view(np.int32), want.view(np.int32))
    return npairs


# walks of 3 nodes on a star: every leaf's walk takes its step 2 on the hub
HUB_PRM = [(8, 1.0, 1.0, 1, 3, 2, 2, 0.025, 1), (8, 0.5, 2.0, 1, 3, 2, 2, 0.025, 1)]

# (dim, p, q, neg) for the batched schedule: every NR template at its lower edge, when full and with idle register slots;
# within each PF class runs of full chunks only ((1 + neg) % PF == 0) and runs that end in a partial chunk
WIDTHS = [(1, 1.0, 1.0, 5), (63, 0.5, 2.0, 6), (64, 1.0, 1.0, 1), (65, 0.5, 2.0, 5), (128, 1.0, 1.0, 6), (129, 0.5, 2.0, 1),
          (192, 1.0, 1.0, 5), (256, 0.5, 2.0, 6), (257, 1.0, 1.0, 1), (384, 0.5, 2.0, 2), (512, 1.0, 1.0, 5),
          (513, 0.5, 2.0, 2), (768, 1.0, 1.0, 1), (1000, 0.5, 2.0, 5), (1024, 1.0, 1.0, 2)]

# (walk_length, batch_walks) with p = q = 1: split 8, 3, 2 and 1
SPLITS = [(20, 5), (3, 64), (2, 64), (1, 64)]


def _within_between(emb, index_of_id, a_ids, b_ids):
    def cos(x, y):
        return float(np.dot(x, y) / (np.linalg.norm(x) * np.linalg.norm(y)))

    A = [emb[index_of_id[i]] for i in a_ids]
    B = [emb[index_of_id[i]] for i in b_ids]
    within = [cos(A[i], A[j]) for i in range(len(A)) for j in range(i + 1, len(A))]
    within += [cos(B[i], B[j]) for i in range(len(B)) for j in range(i + 1, len(B))]
    between = [cos(x, y) for x in A for y in B]
    return np.mean(within), np.mean(between)


@pytest.mark.parametrize("name", sorted(CASES))
def test_oracle_bytes_equal_reference(name):
    z = np.load(os.path.join(G, "node2vec.npz"))
    edges, prm = CASES[name]
    emb, npairs = og.node2vec_train(_graph(edges), *prm)
    assert np.array_equal(emb.view(np.int32), z[name]), name


def test_first_seen_dedup_graph():
    """graph_load_edges (src/node2vec.c:112-138): first-seen indices, both directions, duplicates dropped"""
    g = og.N2vGraph(np.array([5, 5, 7, 2], np.int32), np.array([7, 7, 5, 5], np.int32))
    assert g.n == 3 and g.index_of_id[5] == 0 and g.index_of_id[7] == 1 and g.index_of_id[2] == 2
    assert g.off.tolist() == [0, 2, 3, 4] and g.adj.tolist() == [1, 2, 0, 0]


def test_acceptance_karate_within_gt_between():
    edges, prm = CASES["karate64"]
    g = _graph(edges)
    emb, _ = og.node2vec_train(g, *prm)
    a = [1, 2, 3, 4, 5, 6, 7, 8, 11, 12, 13, 14, 17, 18, 20, 22]
    b = [9, 10, 15, 16, 19, 21, 23, 24, 25, 26, 27, 28, 29, 30, 31, 32, 33, 34]
    w, bt = _within_between(emb, g.index_of_id, a, b)
    assert w > bt


def test_walk_properties():
    edges, _ = CASES["karate64"]
    g = _graph(edges)
    walk, st = og.biased_walk(g, 0, 0.5, 2.0, 40, 12345)
    assert len(walk) == 40 and walk[0] == 0
    for a, b in zip(walk[:-1], walk[1:]):
        assert b in g.adj[g.off[a]:g.off[a + 1]]
    walk2, st2 = og.biased_walk(g, 0, 0.5, 2.0, 40, 12345)
    assert np.array_equal(walk, walk2) and st == st2
    for wl in (1, 2):  # walk[1] is stored before walk_length is looked at (src/node2vec.c:178)
        walk, _ = og.biased_walk(g, 0, 0.5, 2.0, wl, 12345)
        assert len(walk) == wl and walk[0] == 0


def test_live_reference_star_2049_leaves():
    """the oracle against the compiled reference on a hub one past k_n2v_seq's LDS limit (N2V_LDS_DEG = 2048)"""
    if not og.have_ref_graph():
        pytest.skip("compiled reference not present")
    edges = [(0, i) for i in range(1, 2050)]
    for prm in HUB_PRM:
        want = og.ref_node2vec_sql(edges, *prm)
        got, _ = og.node2vec_train(_graph(edges), *prm)
        assert np.array_equal(got.view(np.int32), want.view(np.int32)), prm


def test_width_cases_cover_every_template_and_chunk_shape():
    """WIDTHS reaches every instantiation of n2v_for_width, each with a run of full chunks only and one that ends in a
    partial chunk; SPLITS reaches split 1, 2, 3 and 8."""
    seen = set()
    for dim, p, q, neg in WIDTHS:
        nr, pf, _ = _n2v_template(dim)
        seen.add((nr, (1 + neg) % pf == 0))
    assert seen == {(nr, full) for nr in (1, 2, 4, 8, 16) for full in (True, False)}
    assert {(p, q) for _, p, q, _ in WIDTHS} == {(1.0, 1.0), (0.5, 2.0)}
    assert {_n2v_split(1.0, 1.0, wl, b) for wl, b in SPLITS} == {1, 2, 3, 8}


# ───────────────────────── GPU ─────────────────────────

@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_gpu_sequential_bytes_equal_reference(gpu, name):
    z = np.load(os.path.join(G, "node2vec.npz"))
    edges, prm = CASES[name]
    g = _graph(edges)
    dim, p, q, nw, wl, win, neg, lr, ep = prm
    emb, st = gpu.node2vec_train(g.off, g.adj, dim, p, q, nw, wl, win, neg, lr, ep)
    assert np.array_equal(emb.view(np.int32), z[name]), name
    _, npairs = og.node2vec_train(g, *prm)
    assert st["pairs"] == npairs


@pytest.mark.gpu
def test_gpu_acceptance_two_cliques(gpu):
    edges, prm = CASES["cliques32"]
    g = _graph(edges)
    dim, p, q, nw, wl, win, neg, lr, ep = prm
    emb, _ = gpu.node2vec_train(g.off, g.adj, dim, p, q, nw, wl, win, neg, lr, ep)
    w, b = _within_between(emb, g.index_of_id, [1, 2, 3, 4], [5, 6, 7, 8])
    assert w > b
    assert np.allclose(np.linalg.norm(emb, axis=1), 1.0, atol=1e-5)


@pytest.mark.gpu
def test_gpu_empty_and_invalid(gpu):
    emb, st = gpu.node2vec_train(np.zeros(1, np.int32), np.zeros(0, np.int32), 8)
    assert emb.shape == (0, 8)
    with pytest.raises(Exception):
        gpu.node2vec_train(np.array([0, 1, 2], np.int32), np.array([1, 0], np.int32), 2000)


def _planted_graph():
    from oracle.graph_cases import planted

    s, d, _ = planted(1200, 6, 0.08, 0.002, 7)
    return og.N2vGraph(s, d)


def _block_quality(g, emb):
    blk = np.arange(1200) % 6
    E = emb[g.index_of_id[np.arange(1200)]]
    S = E @ E.T
    same = blk[:, None] == blk[None, :]
    np.fill_diagonal(same, False)
    return float(S[same].mean()), float(S[~same].mean())


def test_batched_schedule_quality_matches_serial_on_cpu():
    g = _planted_graph()
    prm = (32, 1.0, 1.0, 4, 30, 4, 4, 0.025, 2)
    ws, bs = _block_quality(g, og.node2vec_train(g, *prm)[0])
    wb, bb = _block_quality(g, og.node2vec_train_batched(g, *prm, 18)[0])
    assert ws - bs > 0.4 and wb - bb > 0.4 and abs((wb - bb) - (ws - bs)) < 0.15


@pytest.mark.gpu
@pytest.mark.parametrize("prm,batch", [((32, 1.0, 1.0, 4, 30, 4, 4, 0.025, 2), 18), ((32, 1.0, 1.0, 2, 20, 3, 3, 0.025, 1), 1200),
                                       ((70, 0.5, 2.0, 2, 20, 3, 2, 0.05, 1), 7), ((130, 2.0, 0.5, 1, 12, 2, 3, 0.02, 1), 64)])
def test_gpu_batched_bit_exact_vs_oracle_schedule(gpu, prm, batch):
    g = _planted_graph()
    dim, p, q, nw, wl, win, neg, lr, ep = prm
    want, npairs = og.node2vec_train_batched(g, *prm, batch)
    got, st = gpu.node2vec_train(g.off, g.adj, dim, p, q, nw, wl, win, neg, lr, ep, mode=gpu.N2V_BATCHED, batch_walks=batch)
    assert st["pairs"] == npairs
    assert np.array_equal(got.view(np.int32), want.view(np.int32))


@pytest.mark.gpu
def test_gpu_batched_acceptance_blocks(gpu):
    g = _planted_graph()
    emb, st = gpu.node2vec_train(g.off, g.adj, 32, 1.0, 1.0, 4, 30, 4, 4, 0.025, 2, mode=gpu.N2V_BATCHED)
    w, b = _block_quality(g, emb)
    assert w - b > 0.4  # within-block similarity far above between-block (pytests/test_node2vec.py:194-273 in spirit)


@pytest.mark.gpu
def test_gpu_batched_bit_exact_vs_oracle_schedule_8k_nodes(gpu):
    """config 4's kernels at a size between the unit graphs and the bench: ER graph, 8 000 nodes / 80 000 edge draws,
    dim 32, batches of 1024 walks — embedding bits and pair count equal the CPU restatement of the same schedule."""
    rng = np.random.default_rng(3)
    s, d = rng.integers(0, 8000, 80_000), rng.integers(0, 8000, 80_000)
    keep = s != d
    g = og.N2vGraph(s[keep], d[keep])
    prm = (32, 1.0, 1.0, 2, 20, 5, 5, 0.025, 1)
    want, npairs = og.node2vec_train_batched(g, *prm, 1024)
    got, st = gpu.node2vec_train(g.off, g.adj, 32, 1.0, 1.0, 2, 20, 5, 5, 0.025, 1, mode=gpu.N2V_BATCHED, batch_walks=1024)
    assert st["pairs"] == npairs and np.array_equal(got.view(np.int32), want.view(np.int32))


@pytest.mark.gpu
def test_config4_shape_properties_200k_nodes(gpu):
    """BASELINE config 4's parameters (p = q = 1, dim 128, window 5, neg 5, 80-step walks) on a 200k-node / 4M-edge-draw ER
    graph: every embedding is unit length (the reference normalises before its INSERTs), the pair count is the closed
    form for walks that never dead-end, and a second run gives the same bits.  (An ER graph has no community structure for
    the embeddings to separate: the quality checks live in the planted-block tests above.)"""
    rng = np.random.default_rng(42)
    n, m = 200_000, 4_000_000
    s, d = rng.integers(0, n, m), rng.integers(0, n, m)
    keep = s != d
    off, adj = gpu.graph.n2v_csr_from_edges(n, s[keep], d[keep])
    prm = dict(p=1.0, q=1.0, num_walks=2, walk_length=80, window=5, neg_samples=5, learning_rate=0.025, epochs=1)
    emb, st = gpu.node2vec_train(off, adj, 128, mode=gpu.N2V_BATCHED, **prm)
    emb2, st2 = gpu.node2vec_train(off, adj, 128, mode=gpu.N2V_BATCHED, **prm)
    assert np.array_equal(emb.view(np.int32), emb2.view(np.int32)) and st["pairs"] == st2["pairs"]
    nn = len(off) - 1
    assert np.abs(np.linalg.norm(emb, axis=1) - 1.0).max() < 1e-5
    L, W = 80, 5  # pairs of one full-length walk: sum over positions of the clipped window (src/node2vec.c:519-531)
    per_walk = sum(min(L - 1, i + W) - max(0, i - W) for i in range(L))
    assert st["pairs"] == nn * 2 * per_walk  # (mean degree 40: no isolated nodes, no dead ends on an undirected graph)
    assert np.isfinite(emb).all()


@pytest.mark.gpu
@pytest.mark.parametrize("dim", [64, 30, 256, 301])
def test_train_into_index_keeps_the_embeddings_in_hbm_and_builds_the_same_graph(gpu, dim):
    """mn_node2vec_train_into (config 4's "-> hnsw0 index" leg, src/node2vec.c:540-583): the embeddings are trained, normalised
    and handed to the index build inside HBM.  Same embedding bytes as mn_node2vec_train in the same mode, and the index is the
    graph mn_hnsw_build makes from a host copy of those embeddings with the reference's rowids (first-seen index + 1).
    (dim 30 and 301: the index pads rows to a multiple of 4 floats, so the device-to-device hand-off is a strided copy;
    dim 256: the index also keeps its fp16 shadow of the rows.)"""
    from oracle.graph_cases import planted

    s, d, _ = planted(3000, 6, 0.05, 0.001, 11)
    g = og.N2vGraph(s, d)
    want, st1 = gpu.node2vec_train(g.off, g.adj, dim, 1.0, 1.0, 3, 20, 4, 3, 0.025, 1, mode=gpu.N2V_BATCHED, batch_walks=200)
    ix = gpu.HnswIndex(dim, "cosine", 8, 60)
    emb, st = gpu.graph.node2vec_train_into(g.off, g.adj, dim, ix, 1, True, 1.0, 1.0, 3, 20, 4, 3, 0.025, 1, 200)
    assert np.array_equal(emb.view(np.int32), want.view(np.int32)) and st["pairs"] == st1["pairs"]
    ids = np.arange(1, g.n + 1, dtype=np.int64)
    ref = gpu.HnswIndex(dim, "cosine", 8, 60)
    assert ref.build(ids, want, 16, 8192) == 0
    assert ix.node_count == g.n and ix.entry_point == ref.entry_point and ix.max_level == ref.max_level
    assert np.array_equal(ix.export_links(0), ref.export_links(0)) and np.array_equal(ix.export_links(1), ref.export_links(1))
    q = want[:50]
    a, b = ix.search_batch(q, 5, 40), ref.search_batch(q, 5, 40)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.int32), b[1].view(np.int32))
    ix.close()
    ref.close()


# ───────────────────────── GPU: widths, hubs and walk shapes at the edges of the kernels ─────────────────────────

@pytest.mark.gpu
@pytest.mark.parametrize("leaves", [2048, 2049])
@pytest.mark.parametrize("prm", HUB_PRM, ids=["uniform", "pq"])
def test_gpu_sequential_hub_at_the_lds_limit(gpu, leaves, prm):
    """k_n2v_seq keeps a step's running totals in LDS up to N2V_LDS_DEG = 2048 neighbours and in global scratch above
    (the totals are also summed there when p = q = 1).  Every leaf's walk takes a step on the hub."""
    _seq_vs_oracle(gpu, _star(leaves), prm)


@pytest.mark.gpu
@pytest.mark.parametrize("wl", [1, 2])
def test_gpu_sequential_walk_length_1_and_2(gpu, wl):
    """The shortest walks, on a graph with isolated nodes (walks of one node).  A walk of 2 nodes has 2 pairs.  (No reference
    golden: the reference writes walk[1] past its buffer of walk_length ints, src/node2vec.c:178.)"""
    g = _dead_end_graph()
    npairs = _seq_vs_oracle(gpu, g, (16, 0.5, 2.0, 2, wl, 2, 3, 0.025, 1))
    assert npairs == (0 if wl == 1 else 2 * 2 * np.count_nonzero(np.diff(g.off)))


@pytest.mark.gpu
@pytest.mark.parametrize("dim,p,q,neg", WIDTHS)
def test_gpu_batched_every_width_bit_exact(gpu, dim, p, q, neg):
    """k_n2v_walk_grad, k_n2v_apply and k_n2v_apply_centers at every NR template (see WIDTHS), batches of 64 walks of
    203 nodes (the last batch has 11)."""
    _batched_vs_oracle(gpu, _dead_end_graph(), (dim, p, q, 1, 10, 2, neg, 0.025, 1), 64)


def _hub_graph():
    """a ring of 1 500 nodes plus hubs of exactly 512, 513 and 1 500 neighbours on it"""
    n = 1500
    edges = [(i, (i + 1) % n) for i in range(n)] + [(n, i) for i in range(512)] + [(n + 1, i) for i in range(513)]
    return _graph(edges + [(n + 2, i) for i in range(n)])


@pytest.mark.gpu
@pytest.mark.parametrize("dim,neg", [(65, 6), (513, 2)])
@pytest.mark.parametrize("p,q", [(0.5, 2.0), (1.0, 1.0)])
def test_gpu_batched_hubs_at_the_lds_limit(gpu, dim, neg, p, q):
    """The biased walk keeps a step's running totals in LDS up to N2VB_LDS_DEG = 512 neighbours and in per-walk global
    scratch above; p = q = 1 takes the closed form instead.  One dim of each PF class."""
    g = _hub_graph()
    assert sorted(np.diff(g.off))[-3:] == [512, 513, 1500]
    _batched_vs_oracle(gpu, g, (dim, p, q, 1, 8, 2, neg, 0.025, 1), 100)


@pytest.mark.gpu
@pytest.mark.parametrize("dim", [65, 513])
def test_gpu_batched_hub_row_over_64_samples_per_batch(gpu, dim):
    """k_n2v_apply reads a row's samples 64 at a time and folds U of them at once (U = 8 at dim 65, 1 at dim 513).  On a
    star whose leaves have only the hub as neighbour, every walk has the hub at position 1 (the hub's own walk at 0).  With 2
    nodes per walk and window 1, a walk's pairs are (start, hub) and (hub, start): the first gives the hub row exactly one
    sample, its positive (a negative that draws the hub is dropped as the context), the second none (the hub is the
    centre).  So the hub row gets one sample per walk of the batch: 141 = 64 + 64 + 13 in each full batch of 141, and 13 is
    not a multiple of U.  Walks of 6 nodes with window 2 and p != q then give it several per walk."""
    g = _star(299)
    assert _batched_vs_oracle(gpu, g, (dim, 1.0, 1.0, 1, 2, 1, 5, 0.025, 1), 141) == 2 * g.n
    _batched_vs_oracle(gpu, g, (dim, 0.5, 2.0, 1, 6, 2, 2, 0.025, 1), 141)


@pytest.mark.gpu
@pytest.mark.parametrize("dim,neg", [(65, 5), (513, 2)])
@pytest.mark.parametrize("wl,batch", SPLITS)
def test_gpu_batched_split_walks(gpu, dim, neg, wl, batch):
    """`split` wavefronts share one walk, each owning a range of its positions.  Isolated nodes and dead ends end walks
    before most parts start; 203 walks in batches of 64 (or 5) end in a short batch."""
    g = _dead_end_graph()
    npairs = _batched_vs_oracle(gpu, g, (dim, 1.0, 1.0, 2, wl, 3, neg, 0.025, 1), batch)
    if wl <= 2:
        assert npairs == (0 if wl == 1 else 2 * 2 * np.count_nonzero(np.diff(g.off)))


@pytest.mark.gpu
@pytest.mark.parametrize("dim", [65, 513])
@pytest.mark.parametrize("p,q", [(1.0, 1.0), (0.5, 2.0)])
def test_gpu_batched_walk_longer_than_4096(gpu, dim, p, q):
    edges, _ = CASES["cliques_walk4100"]
    _batched_vs_oracle(gpu, _graph(edges), (dim, p, q, 1, 4100, 2, 2, 0.025, 1), 8)
