"""Every vector kernel picks its code by the row length ld = round_up(dim, 4): the wave order's chunk count NCH (pick_nch:
1, 2, 3, 4, 6, 8, and 0 = the generic loop above 2048 floats), the reference order's float4 walk (rows of dim >> 4 >= 12 blocks,
taken in blocks of 12, 8, 4, 2, 1, then chains, then a dim % 4 tail), the fp16 shadow filter (ld >= 192, ld % 64 == 0) and the
lone-search / lone-insert kernels' per-wavefront LDS tile (4 rows, 2 rows or none, by what fits the device's opt-in LDS).  Each
entry of DIMS reaches a stated combination; the tests check every kernel family against the CPU oracle at those row lengths,
bit for bit (ids, distance bits, counts, graphs) — and the geometry each entry claims is asserted from MN_LAT_DEBUG, not assumed.
Family (f) is the exact search (csrc/mn_exact.hip): k_exact_rescore<ORDER, NCH> and k_exact_valu<ORDER, NCH> at every NCH in both
orders, the re-score's two launch shapes (4 queries per workgroup while 16·ld bytes fit 32 KB, one above: ld > 2048) and
k_exact_mfma's partial last 32-float stage (ld % 32 != 0).
Family (g) is the self-join of the same kernels (mn_hnsw_knn_graph): k_exact_rescore<ORDER, NCH, true>, k_exact_valu<ORDER, NCH, ExSelf>
and k_exact_prep_q<ORDER, true> at the row lengths of family (f), in query batches of 128 + 128 + 44 slots."""
import os
import subprocess
import sys

import numpy as np
import pytest

import test_knn_graph as kg
from test_exact_search import check, distances, exact, reference
from util import check_topk_f64, gauss, same_bits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
METRICS = ["l2", "cosine", "inner_product"]

# dim: (wave NCH, quad residue (dim >> 4) % 12, dim % 4, fp16 shadow, k_beam_coop tile rows, k_insert_seq tile rows)
# tile rows: reference order, M = 8, 160 KB of opt-in LDS per workgroup (MI355X)
DIMS = {
    192: (1, 0, 0, True, 0, 0),     # shortest row with the shadow; quad walk from 12 blocks on; no tile below 256
    208: (1, 1, 0, False, 0, 0),    # ld % 64 != 0: shadow off just above 192
    226: (1, 2, 2, False, 0, 0),    # dim % 4 = 2
    255: (1, 3, 3, True, 4, 4),     # ld 256: shadow on, first dim with tiles; dim % 4 = 3
    275: (2, 5, 3, False, 4, 4),    # NCH 2
    300: (2, 6, 0, False, 4, 4),
    345: (2, 9, 1, False, 4, 4),    # dim % 4 = 1
    509: (2, 7, 1, True, 4, 4),     # ld 512, tail of one element
    551: (3, 10, 3, False, 4, 4),   # NCH 3
    641: (3, 4, 1, False, 4, 4),
    708: (3, 8, 0, False, 4, 4),
    953: (4, 11, 1, False, 2, 2),   # NCH 4; the 4-row tile no longer fits: 2 rows
    1021: (4, 3, 1, True, 2, 2),    # ld 1024 with a tail
    1024: (4, 4, 0, True, 2, 2),
    1283: (6, 8, 3, False, 2, 2),   # NCH 6
    1536: (6, 0, 0, True, 2, 0),    # k_beam_coop still 2 rows, k_insert_seq none
    1999: (8, 4, 3, False, 0, 0),   # NCH 8; no tile in either kernel
    2048: (8, 8, 0, True, 0, 0),    # longest row of the chunked wave walk
    2050: (0, 8, 2, False, 0, 0),   # NCH 0: the generic loop
    3072: (0, 0, 0, True, 0, 0),
    4096: (0, 4, 0, True, 0, 0),
}
# family (c): at least one dim per NCH instance and per tile geometry of both lone kernels
BUILD_DIMS = [255, 300, 708, 1024, 1283, 1536, 1999, 2050]
# brute force: k_bruteforce (MN_BRUTE=valu) at every NCH, k_brute_mfma at rows that are not whole 32-float column tiles
BRUTE_VALU_DIMS = [192, 300, 708, 1024, 1536, 2048, 3072]
BRUTE_MFMA_DIMS = [226, 345, 953, 1283, 2050]
# family (f): NCH 1, 2, 3, 4, 6, 8, 8, 0, 0; ld 228, 348, 708, 1284 and 2052 are not whole 32-float stages of k_exact_mfma; 2048 is the
# last row re-scored 4 queries per workgroup, 2050 the first re-scored one per workgroup
EXACT_DIMS = [226, 345, 708, 1021, 1283, 1999, 2048, 2050, 4096]
# family (g): the same row lengths; every row is a query, in batches of KNN_BATCH slots: two whole ones and a ragged last tile
KNN_DIMS = EXACT_DIMS
KNN_N, KNN_BATCH = 300, 128


def _ld(dim):
    return (dim + 3) & ~3


def _nch(ld):
    need = (ld + 255) // 256
    return next((c for c in (1, 2, 3, 4, 6, 8) if need <= c), 0)


def test_table_states_what_the_dispatch_picks_and_reaches_every_path():
    """CPU-side: the table's NCH / residue / tail / shadow columns are what the launchers compute, and together they cover
    every instance named in the module docstring (the tile columns are checked on the device: test_lone_kernel_geometry)."""
    for dim, (nch, res, tail, shadow, coop, seq) in DIMS.items():
        ld = _ld(dim)
        assert nch == _nch(ld), dim
        assert dim >> 4 >= 12 and res == (dim >> 4) % 12, dim
        assert tail == dim % 4, dim
        assert shadow == (ld >= 192 and ld % 64 == 0), dim
    cols = list(zip(*DIMS.values()))
    assert set(cols[0]) == {0, 1, 2, 3, 4, 6, 8}
    assert set(cols[1]) == set(range(12))
    assert set(cols[2]) == {0, 1, 2, 3}
    assert {DIMS[d][3] for d in DIMS if d < 256} == {True, False} and {DIMS[d][3] for d in DIMS if d > 1024} == {True, False}
    assert all(DIMS[d][3] for d in (1024, 1536, 3072, 4096))
    assert set(cols[4]) == {0, 2, 4} and set(cols[5]) == {0, 2, 4}
    assert {DIMS[d][0] for d in BUILD_DIMS} == {0, 1, 2, 3, 4, 6, 8}
    assert {DIMS[d][4] for d in BUILD_DIMS} == {0, 2, 4} and {DIMS[d][5] for d in BUILD_DIMS} == {0, 2, 4}
    assert {DIMS[d][0] for d in BRUTE_VALU_DIMS} == {0, 1, 2, 3, 4, 6, 8}
    assert all(_ld(d) % 32 for d in BRUTE_MFMA_DIMS)
    assert {DIMS[d][0] for d in EXACT_DIMS} == {0, 1, 2, 3, 4, 6, 8}
    assert any(_ld(d) % 32 != 0 for d in EXACT_DIMS)
    assert {_ld(d) * 16 <= 32768 for d in EXACT_DIMS} == {True, False}
    assert _ld(2048) * 16 == 32768 and 2050 in EXACT_DIMS  # both sides of the re-score's switch, at the switch
    assert {DIMS[d][0] for d in KNN_DIMS} == {0, 1, 2, 3, 4, 6, 8}
    assert {_ld(d) * 16 <= 32768 for d in KNN_DIMS} == {True, False}
    assert KNN_BATCH % 128 == 0 and KNN_N // KNN_BATCH == 2 and 0 < KNN_N % KNN_BATCH < 128  # 128 + 128 + 44 query slots


def _orders(gpu, orc):
    return (("sse", gpu.ORDER_SSE, orc.ORDER_SSE), ("wave", gpu.ORDER_WAVE, orc.ORDER_WAVE))


# ───────────────────────── (a) vec_dist_batch ─────────────────────────

@pytest.mark.gpu
@pytest.mark.parametrize("dim", list(DIMS))
def test_dist_batch(gpu, orc, dim):
    X = gauss(150, dim, 7)
    q = gauss(1, dim, 8)[0]
    X[3] = 0.0
    X[5] = q
    for metric in METRICS:
        for tag, go, oo in _orders(gpu, orc):
            got = gpu.vec_dist_batch(metric, q, X, go)
            assert same_bits(got, orc.dist_batch(metric, q, X, oo)), (metric, tag)
        ref = orc.dist_batch(metric, q, X, orc.ORDER_SSE)
        fast = gpu.vec_dist_batch(metric, q, X, gpu.ORDER_WAVE)
        qn, xn = np.linalg.norm(q), np.linalg.norm(X, axis=1)
        floor = {"cosine": np.ones_like(xn), "inner_product": qn * xn, "l2": qn * qn + xn * xn}[metric]
        assert np.max(np.abs(fast - ref) / np.maximum(np.abs(ref), floor + 1e-30)) < 1e-5, metric


# ───────────────────────── (b) search over a fixed oracle graph ─────────────────────────

def _search_case(dim):
    n = 700 if dim <= 1024 else 400
    X = gauss(n, dim, 40 + dim)
    X[n // 2:n // 2 + 12] = X[:12]  # exact duplicates: distance ties
    ids = np.arange(n, dtype=np.int64) * 5 + 2
    Q = np.concatenate([gauss(124, dim, 41 + dim), X[:6] + 0.0])  # 130 queries: more than 128 (k_beam)
    return n, X, ids, Q


@pytest.mark.gpu
@pytest.mark.parametrize("dim", list(DIMS))
def test_search_three_ways(gpu, orc, monkeypatch, dim):
    """k_beam (filter on and off), k_beam_coop (<= 128 queries) and one query at a time: the oracle's answers every time"""
    n, X, ids, Q = _search_case(dim)
    n_lone = 4 if dim > 1024 else 8
    for metric in METRICS:
        for tag, go, oo in _orders(gpu, orc):
            o = orc.Oracle(dim, metric, 8, 32, order=oo)
            assert o.insert_many(ids, X) == 0
            for d in ids[np.random.default_rng(dim).choice(n, n // 20, replace=False)]:
                o.delete(int(d))
            g = gpu.HnswIndex(dim, metric, 8, 32, order=go)
            g.load_graph_from(o, ids, X)
            for k, ef in ((10, 10), (10, 64), (20, 300)):  # ef 300 > MN_RES_LDS: the result heap spills
                key = (metric, tag, k, ef)
                wi, wd, wc = o.search_many(Q, k, ef)
                out = []
                for off in (False, True):
                    if off:
                        monkeypatch.setenv("MN_LOWPREC_FILTER", "0")
                    else:
                        monkeypatch.delenv("MN_LOWPREC_FILTER", raising=False)
                    out.append((g.search_batch(Q, k, ef), g.last_launch()))
                monkeypatch.delenv("MN_LOWPREC_FILTER", raising=False)
                for (gi, gd, gc), _ in out:
                    assert np.array_equal(gc, wc), key
                    assert np.array_equal(gi, wi), key
                    assert same_bits(gd, wd), key
                (_, st), (_, sw) = out
                assert (st["last_n_dist"], st["last_n_expanded"]) == (sw["last_n_dist"], sw["last_n_expanded"]), key
                assert sw["last_n_exact_rows"] == sw["last_n_dist"], key
                assert st["last_n_exact_rows"] <= st["last_n_dist"], key
                ci, cd, cc = g.search_batch(Q[:40], k, ef)  # k_beam_coop
                assert np.array_equal(cc, wc[:40]) and np.array_equal(ci, wi[:40]) and same_bits(cd, wd[:40]), key
                for qi in list(range(n_lone // 2)) + list(range(len(Q) - n_lone // 2, len(Q))):
                    si, sd = g.search(Q[qi], k, ef)
                    assert np.array_equal(si, wi[qi, :wc[qi]]) and same_bits(sd, wd[qi, :wc[qi]]), key + (qi,)
            g.close()


# ───────────────────────── (c) graph construction, (d) edges_of ─────────────────────────

def _check_edges(g, orc, metric, oo, ids, X, id0):
    pick = ids[::max(1, len(ids) // 25)]
    src, dst, lvl, dist = g.edges_of(pick)
    assert len(src) > 0
    for s_, d_, x in zip(src, dst, dist):
        want = orc.distance(metric, X[int(s_) - id0], X[int(d_) - id0], oo)
        assert same_bits(np.float32(x), want), (metric, int(s_), int(d_))


@pytest.mark.gpu
@pytest.mark.parametrize("dim", BUILD_DIMS)
def test_build_three_ways(gpu, orc, dim):
    """k_insert_seq (one insert at a time), the speculative windows (insert_batch SEQUENTIAL) and the batched build
    (k_beam<BUILD> + k_link_reverse) give the oracle's graph; k_edge_rows gives the oracle's edge distances"""
    n = 320 if dim <= 1024 else 240
    metric = METRICS[BUILD_DIMS.index(dim) % 3]
    X = gauss(n, dim, 60 + dim)
    X[200:206] = X[10:16]  # ties in the prunes
    id0 = 1000
    ids = np.arange(id0, id0 + n, dtype=np.int64)
    for tag, go, oo in _orders(gpu, orc):
        key = (metric, tag)
        o = orc.Oracle(dim, metric, 8, 32, order=oo)
        assert o.insert_many(ids, X) == 0
        want = o.graph(ids)
        g = gpu.HnswIndex(dim, metric, 8, 32, order=go)
        for i in range(n):
            assert g.insert(int(ids[i]), X[i]) == 0
        assert g.graph(ids) == want, key + ("insert",)
        _check_edges(g, orc, metric, oo, ids, X, id0)
        g.close()
        g = gpu.HnswIndex(dim, metric, 8, 32, order=go)
        assert g.insert_batch(ids[:5], X[:5], gpu.BUILD_SEQUENTIAL) == 0
        assert g.insert_batch(ids[5:], X[5:], gpu.BUILD_SEQUENTIAL) == 0
        assert g.graph(ids) == want, key + ("sequential",)
        g.close()
        ob = orc.Oracle(dim, metric, 8, 32, order=oo)
        g = gpu.HnswIndex(dim, metric, 8, 32, order=go)
        pos = 0
        for b in (1, 2, 9, 40, 97, n):
            b = min(b, n - pos)
            assert ob.insert_batch(ids[pos:pos + b], X[pos:pos + b]) == 0
            assert g.insert_batch(ids[pos:pos + b], X[pos:pos + b], gpu.BUILD_BATCHED) == 0
            pos += b
        assert pos == n
        assert g.graph(ids) == ob.graph(ids), key + ("batched",)
        _check_edges(g, orc, metric, oo, ids, X, id0)
        g.close()


@pytest.mark.gpu
def test_wide_rows_above_1024(gpu, orc):
    """M = 40: lists of 80 links, walked 64 at a time (the WIDE kernels), at a row of NCH 6"""
    dim, n, M = 1283, 260, 40
    X = gauss(n, dim, 91)
    ids = np.arange(1, n + 1, dtype=np.int64)
    for tag, go, oo in _orders(gpu, orc):
        o = orc.Oracle(dim, "l2", M, 48, order=oo)
        assert o.insert_many(ids, X) == 0
        g = gpu.HnswIndex(dim, "l2", M, 48, order=go)
        for i in range(n):
            assert g.insert(int(ids[i]), X[i]) == 0
        assert g.graph(ids) == o.graph(ids), tag
        Q = gauss(20, dim, 92)
        wi, wd, wc = o.search_many(Q, 10, 64)
        gi, gd, gc = g.search_batch(Q, 10, 64)
        assert np.array_equal(gi, wi) and same_bits(gd, wd), tag
        g.close()
        ob = orc.Oracle(dim, "l2", M, 48, order=oo)
        g = gpu.HnswIndex(dim, "l2", M, 48, order=go)
        for lo, hi in ((0, 1), (1, 30), (30, n)):
            assert ob.insert_batch(ids[lo:hi], X[lo:hi]) == 0
            assert g.insert_batch(ids[lo:hi], X[lo:hi], gpu.BUILD_BATCHED) == 0
        assert g.graph(ids) == ob.graph(ids), tag
        g.close()


# ───────────────────────── the lone kernels' LDS geometry, as the launchers report it ─────────────────────────

_GEOM_SCRIPT = r"""
import os, sys
import numpy as np
sys.path.insert(0, os.environ["MN_ROOT"])
import muninn_amd
pkg = muninn_amd.pkg
for dim in [int(d) for d in sys.argv[1:]]:
    X = np.random.default_rng(dim).standard_normal((40, dim)).astype(np.float32)
    g = pkg.HnswIndex(dim, "l2", 8, 32)
    sys.stderr.write("DIM %d\n" % dim)
    sys.stderr.flush()
    for i in range(40):
        assert g.insert(i + 1, X[i]) == 0
    g.search(X[0], 5, 16)
    g.close()
    sys.stderr.flush()
print("OK")
"""


def lone_kernel_geometry(dims):
    """{dim: ({k_beam_coop tile rows}, {k_insert_seq tile rows})} as MN_LAT_DEBUG reports them, from a child process"""
    env = dict(os.environ, MN_ROOT=ROOT, MN_LAT_DEBUG="1")
    r = subprocess.run([sys.executable, "-c", _GEOM_SCRIPT] + [str(d) for d in dims], env=env, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0 and "OK" in r.stdout, r.stderr[-1500:]
    seen, cur = {}, None
    for line in r.stderr.splitlines():
        if line.startswith("DIM "):
            cur = int(line.split()[1])
            seen[cur] = (set(), set())
        elif line.startswith("[mn] k_beam_coop: distance tile of ") and cur is not None:
            seen[cur][0].add(int(line.split("distance tile of ")[1].split()[0]))
        elif line.startswith("[mn] k_insert_seq: distance tile of ") and cur is not None:
            seen[cur][1].add(int(line.split("distance tile of ")[1].split()[0]))
    return seen


@pytest.mark.gpu
def test_lone_kernel_geometry(gpu):
    """every entry's tile columns are what the launchers pick on this device (reference order, M = 8)"""
    seen = lone_kernel_geometry(list(DIMS))
    for dim, (_, _, _, _, coop, seq) in DIMS.items():
        assert seen[dim] == ({coop}, {seq}), (dim, seen[dim], (coop, seq))


# ───────────────────────── (e) brute force against float64 ─────────────────────────

def _brute(gpu, dim, metric, order, nq, k, valu, monkeypatch):
    n = 1200
    X = gauss(n, dim, 100 + dim)
    X[17] = X[3]
    Q = gauss(nq, dim, 101 + dim)
    Q[0] = X[3]
    ids = np.arange(100, 100 + n, dtype=np.int64)
    g = gpu.HnswIndex(dim, metric, 8, 32, order=order)
    assert g.insert_batch(ids, X, gpu.BUILD_BATCHED) == 0
    dels = [105, 140, 1000]
    for dl in dels:
        assert g.delete(dl) == 0
    dq = g.dev_malloc(Q.nbytes)
    g.dev_upload(dq, Q)
    if valu:
        monkeypatch.setenv("MN_BRUTE", "valu")
    got = g.bruteforce_topk(dq, nq, k)
    monkeypatch.delenv("MN_BRUTE", raising=False)
    g.dev_free(dq)
    g.close()
    check_topk_f64(got, X, Q, ids, np.array(dels, np.int64), k, metric)
    assert set(got[0][:2].tolist()) == {103, 117}  # the duplicated row, both copies


@pytest.mark.gpu
@pytest.mark.parametrize("dim", BRUTE_VALU_DIMS)
def test_bruteforce_valu_against_f64(gpu, monkeypatch, dim):
    for i, metric in enumerate(METRICS):
        order = gpu.ORDER_WAVE if i < 2 else gpu.ORDER_SSE
        _brute(gpu, dim, metric, order, 24, 10, True, monkeypatch)


@pytest.mark.gpu
@pytest.mark.parametrize("dim", BRUTE_MFMA_DIMS)
def test_bruteforce_mfma_against_f64(gpu, monkeypatch, dim):
    for metric in METRICS:
        _brute(gpu, dim, metric, gpu.ORDER_SSE, 140, 16, False, monkeypatch)


# ───────────────────────── (f) exact search ─────────────────────────

@pytest.mark.gpu
@pytest.mark.parametrize("dim", EXACT_DIMS)
def test_exact_search(gpu, orc, monkeypatch, dim):
    """candidate pass + re-score (default), the walk forced (MN_EXACT=valu) and the walk by k (33 > 32): the oracle's k nearest
    live rows under (d, slot), ids and distance bits, for every metric in both orders"""
    n, nq = 300, 40  # two full 128-row tiles and a ragged one
    X = gauss(n, dim, 120 + dim)
    X[17] = X[3]  # exact duplicate rows: the lower slot comes first
    X[5] = 0.0
    Q = gauss(nq, dim, 121 + dim)
    Q[0] = X[3]
    ids = np.arange(100, 100 + n, dtype=np.int64)
    for metric in METRICS:
        for tag, go, oo in _orders(gpu, orc):
            D = distances(orc, metric, oo, X, Q)
            top1 = int(np.argmin(D[1]))  # a would-be top-1 goes
            assert top1 not in (3, 17), (metric, tag)
            dead = sorted({top1, 40, 290, 150} - {3, 17}, key=lambda s: s != top1)[:3]
            assert len(dead) == 3 and top1 in dead
            g = gpu.HnswIndex(dim, metric, 8, 32, order=go)
            assert g.insert_batch(ids, X, gpu.BUILD_BATCHED) == 0
            for d in dead:
                assert g.delete(int(ids[d])) == 0
            live = np.setdiff1d(np.arange(n), dead)
            for k, env in ((10, {}), (10, {"MN_EXACT": "valu"}), (33, {})):
                key = (metric, tag, k, env)
                want = reference(orc, metric, oo, X, ids, live, Q, k, D)
                assert ids[top1] not in want[0][1], key
                assert metric == "inner_product" or list(want[0][0][:2]) == [103, 117], key
                for name, v in env.items():
                    monkeypatch.setenv(name, v)
                got, st = exact(g, Q, k)
                for name in env:
                    monkeypatch.delenv(name)
                check(got, want, key)
                assert st["n_mfma_queries"] == (nq if k <= 32 and not env else 0), (key, st)
            g.close()


# ───────────────────────── (g) the exact k-NN graph of the index's own rows ─────────────────────────

@pytest.mark.gpu
@pytest.mark.parametrize("dim", KNN_DIMS)
def test_knn_graph(gpu, orc, monkeypatch, dim):
    """the self-join's candidate pass + re-score (default), its walk forced (MN_EXACT=valu) and its walk by k (33 > 32), in three
    query batches: test_knn_graph's reference (every live row's other live rows under (d, slot)), ids, distance bits and counts,
    count -1 at the deleted slots, for every metric in both orders"""
    X = gauss(KNN_N, dim, 130 + dim)
    X[17] = X[3]  # exact duplicate rows: each is the other's neighbour, the lower slot first among ties
    ids = np.arange(100, 100 + KNN_N, dtype=np.int64)
    for metric in METRICS:
        for tag, go, oo in _orders(gpu, orc):
            assert go == oo  # (Case carries one order for the oracle's distances and the index)
            c = kg.Case(orc, metric, oo, X, ids)
            d1 = c.D[1].copy()
            d1[1] = np.inf
            top1 = int(np.argmin(d1))  # row 1's would-be nearest goes, and a slot of the ragged last batch
            c.set_dead({top1, 40, 290} - {3, 17})
            n_live = len(c.live)
            assert n_live == KNN_N - len(c.dead) and len(c.dead) in (2, 3)
            g = kg.make_index(gpu, c)
            for k, path in ((10, {}), (10, {"MN_EXACT": "valu"}), (33, {})):
                key = (metric, tag, k, path)
                want = c.reference(k)
                assert (want[2][c.dead] == -1).all() and (want[2][c.live] == k).all(), key
                assert top1 in (3, 17) or ids[top1] not in want[0][1], key
                with kg.env(monkeypatch, path, {"MN_KNN_BATCH": str(KNN_BATCH)}):
                    got, st = kg.knn(g, k)
                kg.check(got, want, key)
                assert st["n_queries"] == n_live, (key, st)
                assert st["n_mfma_queries"] == (n_live if k <= 32 and not path else 0), (key, st)
            g.close()


# ───────────────────────── the dimension ceiling ─────────────────────────

@pytest.mark.gpu
def test_dimension_ceiling(gpu, orc):
    """mn_hnsw_max_dim: every kernel fits at the limit (a small index builds three ways and searches bit-exact against the
    oracle); create refuses limit + 4 with a message naming the limit, before anything is launched"""
    M = 8
    lim = gpu.max_dim(M)
    assert lim >= max(DIMS) and lim % 4 == 0, lim
    with pytest.raises(gpu.MuninnHipError, match=f"limit of {lim}"):
        gpu.HnswIndex(lim + 4, "l2", M, 32)
    n, dim = 48, lim
    X = gauss(n, dim, 5)
    X[30] = X[2]
    ids = np.arange(1, n + 1, dtype=np.int64)
    Q = np.concatenate([gauss(3, dim, 6), X[:2] + 0.0])
    for metric, (tag, go, oo) in zip(("l2", "cosine"), _orders(gpu, orc)):
        o = orc.Oracle(dim, metric, M, 32, order=oo)
        assert o.insert_many(ids, X) == 0
        g = gpu.HnswIndex(dim, metric, M, 32, order=go)
        for i in range(6):
            assert g.insert(int(ids[i]), X[i]) == 0
        assert g.insert_batch(ids[6:], X[6:], gpu.BUILD_SEQUENTIAL) == 0
        assert g.graph(ids) == o.graph(ids), tag
        wi, wd, wc = o.search_many(Q, 5, 40)
        gi, gd, gc = g.search_batch(Q, 5, 40)
        assert np.array_equal(gi, wi) and same_bits(gd, wd), tag
        si, sd = g.search(Q[0], 5, 40)
        assert np.array_equal(si, wi[0]) and same_bits(sd, wd[0]), tag
        src, dst, lvl, dist = g.edges_of(ids[:4])
        assert all(same_bits(np.float32(x), orc.distance(metric, X[s_ - 1], X[d_ - 1], oo)) for s_, d_, x in zip(src, dst, dist))
        g.close()
        ob = orc.Oracle(dim, metric, M, 32, order=oo)
        g = gpu.HnswIndex(dim, metric, M, 32, order=go)
        for lo, hi in ((0, 1), (1, 9), (9, n)):
            assert ob.insert_batch(ids[lo:hi], X[lo:hi]) == 0
            assert g.insert_batch(ids[lo:hi], X[lo:hi], gpu.BUILD_BATCHED) == 0
        assert g.graph(ids) == ob.graph(ids), tag
        g.close()


@pytest.mark.gpu
def test_dist_batch_past_64kb_of_lds(gpu, orc):
    """k_dist_batch stages the query and a row (8·ld bytes): just below 8192 floats without the opt-in, just above with it,
    and far beyond what any device grants: -1 with a message, nothing launched"""
    for dim in (8188, 8196):
        X = gauss(40, dim, 3)
        q = gauss(1, dim, 4)[0]
        X[1] = 0.0
        X[2] = q
        for metric in METRICS:
            for tag, go, oo in _orders(gpu, orc):
                assert same_bits(gpu.vec_dist_batch(metric, q, X, go), orc.dist_batch(metric, q, X, oo)), (dim, metric, tag)
    with pytest.raises(gpu.MuninnHipError, match="bytes of LDS"):
        gpu.vec_dist_batch("l2", np.ones(300_000, np.float32), np.ones((2, 300_000), np.float32))
