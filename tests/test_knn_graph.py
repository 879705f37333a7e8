"""The exact k-NN graph of an index's own rows (mn_hnsw_knn_graph, csrc/mn_exact.hip) against the CPU oracle's
distances, bit for bit.

Contract: for a live slot s the answer is the k smallest rows under (d ascending as floats, slot ascending) among the live
slots t != s with d <= max_distance, d = the index's own distance with row s's stored vector as the query
(oracle.orc.dist_batch in the index's order gives its bits).  The exclusion is by slot: a duplicate of s is a neighbour.
Through the raw call a deleted slot has count -1.  Every path gives that one answer: the default (matrix-core candidate pass
with the row store as both operands, re-score, certificate), MN_EXACT=valu (the index's inner loop over every row),
MN_EXACT_SLACK=0 (every certificate fails, every query falls back), each in one query batch and in several."""
import numpy as np
import pytest

from util import gauss, same_bits

pytestmark = pytest.mark.gpu

N = 1200  # all rows are queries: two row chunks of 640 and 560 rows (ex_chunks), the last row tile and the last query tile ragged
KS = (1, 10, 32, 33)  # 32 / 33: the last k the matrix-core pass serves and the first it does not
CONFIGS = [(m, d, o) for m in ("l2", "cosine", "inner_product") for d, o in ((33, 0), (128, 1), (768, 0))]
PATHS = ({}, {"MN_EXACT": "valu"}, {"MN_EXACT_SLACK": "0"})
BATCHES = ({}, {"MN_KNN_BATCH": "512"})  # 512 + 512 + 176 query slots, the last batch ending in a ragged tile
INF = np.float32(np.inf)


class Case:
    """One index's rows, the oracle's distance of every row to every row (computed once) and every live row's other live rows
    in (d, slot) order: the reference answer for any k and radius is a prefix of that."""

    def __init__(self, orc, metric, order, X, ids, dead=()):
        self.metric, self.order, self.X, self.ids = metric, order, X, ids
        n = len(X)
        self.D = np.stack([orc.dist_batch(metric, X[i], X, order) for i in range(n)]) if n else np.zeros((0, 0), np.float32)
        self.set_dead(dead)

    def set_dead(self, dead):
        n = len(self.X)
        self.dead = np.array(sorted(dead), np.int64)
        self.live = np.setdiff1d(np.arange(n), self.dead)
        self.ranked = {}
        for s in self.live:
            others = self.live[self.live != s]
            d = self.D[s][others]
            o = np.lexsort((others, d))
            self.ranked[int(s)] = (others[o], d[o])

    def reference(self, k, r=INF):
        """by slot: (ids [n][k], dists [n][k], counts [n]), count -1 at the deleted slots"""
        n = len(self.X)
        ri = np.full((n, k), -1, np.int64)
        rd = np.full((n, k), np.inf, np.float32)
        rc = np.full(n, -1, np.int32)
        for s, (slots, d) in self.ranked.items():
            keep = np.nonzero(d <= r)[0][:k]
            ri[s, :len(keep)] = self.ids[slots[keep]]
            rd[s, :len(keep)] = d[keep]
            rc[s] = len(keep)
        return ri, rd, rc


_cases = {}


def gaussian_case(orc, metric, dim, order):
    """The data of tests 1 and 2: Gaussian rows, one exact duplicate pair, three deleted rows — one of them row 1's nearest."""
    key = (metric, dim, order)
    if key not in _cases:
        X = gauss(N, dim, 21)
        X[17] = X[3]
        ids = np.arange(100, 100 + N, dtype=np.int64)
        c = Case(orc, metric, order, X, ids)
        d1 = c.D[1].copy()
        d1[1] = np.inf
        c.top1 = int(np.argmin(d1))
        c.set_dead({c.top1, 5, 1040} - {3, 17})
        _cases[key] = c
    return _cases[key]


def make_index(gpu, c):
    g = gpu.HnswIndex(c.X.shape[1], c.metric, 8, 40, order=c.order)
    if len(c.X):
        assert g.insert_batch(c.ids, c.X, gpu.BUILD_BATCHED) == 0
    for d in c.dead:
        assert g.delete(int(c.ids[d])) == 0
    return g


def knn(g, k, r=None):
    """the raw call + the free check of the bound's derivation: no re-scored row lies below its bound"""
    out = g.knn_graph_slots(k, r)
    st = g.last_exact()
    assert st["n_bound_violations"] == 0, st
    return out, st


def check(got, want, what):
    (gi, gd, gc), (wi, wd, wc) = got, want
    assert np.array_equal(gc, wc), (what, np.nonzero(gc != wc)[0][:8])
    assert np.array_equal(gi, wi), (what, np.nonzero((gi != wi).any(axis=1))[0][:8])
    assert same_bits(gd, wd), what


class env:
    def __init__(self, monkeypatch, *dicts):
        self.mp, self.vars = monkeypatch, {k: v for d in dicts for k, v in d.items()}

    def __enter__(self):
        for k, v in self.vars.items():
            self.mp.setenv(k, v)

    def __exit__(self, *a):
        for k in self.vars:
            self.mp.delenv(k)


# ───────────────────────── 1. one answer on every path ─────────────────────────

@pytest.mark.parametrize("metric,dim,order", CONFIGS)
def test_every_path_one_answer(gpu, orc, monkeypatch, metric, dim, order):
    c = gaussian_case(orc, metric, dim, order)
    g = make_index(gpu, c)
    n_live = len(c.live)
    assert n_live == N - len(c.dead) and len(c.dead) in (2, 3)
    for k in KS:
        want = c.reference(k)
        assert c.top1 in (3, 17) or c.ids[c.top1] not in want[0][1]  # row 1's would-be nearest is gone
        assert (want[2][c.dead] == -1).all() and (want[2][c.live] == k).all()
        if metric != "inner_product":  # the duplicate is a neighbour like any other, and the nearest one
            assert want[0][3][0] == c.ids[17] and want[0][17][0] == c.ids[3]
        for path in PATHS:
            for batch in BATCHES:
                with env(monkeypatch, path, batch):
                    got, st = knn(g, k)
                what = (k, path, batch)
                check(got, want, what)
                assert st["n_queries"] == n_live, (what, st)
                if "MN_EXACT" in path or k > 32:
                    assert st["n_mfma_queries"] == 0 and st["n_fallback_queries"] == 0, (what, st)
                elif "MN_EXACT_SLACK" in path:
                    # a list of exactly k rows: the k-th distance is never below the largest bound of the list
                    assert st["n_mfma_queries"] == n_live and st["n_fallback_queries"] == n_live, (what, st)
                else:
                    # the queries are rows of the same Gaussian set as the rows: the gap between the k-th and the (k+16)-th
                    # distance is at least 6.6 bound widths of 16 dim 2^-24 scale at dim 768 and over 50 at dim <= 200 — a
                    # sound bound of ordinary width certifies them (the cap of test_exact_search's three-paths test)
                    assert st["n_mfma_queries"] == n_live and st["n_fallback_queries"] <= 0.05 * n_live, (what, st)
                    assert st["n_rescored_rows"] == n_live * min(k + 16, n_live - 1), (what, st)
    g.close()


# ───────────────────────── 2. the radius ─────────────────────────

@pytest.mark.parametrize("metric,dim,order", CONFIGS)
def test_radius(gpu, orc, monkeypatch, metric, dim, order):
    c = gaussian_case(orc, metric, dim, order)
    g = make_index(gpu, c)
    n_live, k = len(c.live), 10
    full = c.reference(k)
    tenth = full[1][c.live, k - 1]
    r_med = np.float32(np.median(tenth))
    r_dup = c.D[3][17]  # the exact bits of the distance between the duplicate rows
    assert same_bits(r_dup, c.D[17][3])
    r_below = np.nextafter(r_dup, -INF)
    r_none = np.float32(c.D.min() - 1.0)
    for name, r in (("median", r_med), ("dup", r_dup), ("below dup", r_below), ("none", r_none)):
        want = c.reference(k, r)
        if name == "median":
            short = (want[2][c.live] < k).sum()
            assert 0.3 * n_live < short < 0.7 * n_live
        elif name == "dup":  # d <= r keeps the pair
            assert c.ids[17] in want[0][3] and c.ids[3] in want[0][17]
        elif name == "below dup":
            assert c.ids[17] not in want[0][3] and c.ids[3] not in want[0][17]
        else:
            assert (want[2][c.live] == 0).all()
        for path in PATHS:
            with env(monkeypatch, path):
                got, st = knn(g, k, r)
            check(got, want, (name, path))
            assert st["n_queries"] == n_live
            if name == "median" and not path:
                # the cut reached the candidate pass: rows with lb > r are refused there, so most lists end short of K' = 26
                assert st["n_mfma_queries"] == n_live and st["n_rescored_rows"] < n_live * 26, st
    # an explicit +inf is no cut
    check(knn(g, k, np.inf)[0], full, "inf")
    g.close()


# ───────────────────────── 3. ties past the list ─────────────────────────

@pytest.mark.parametrize("metric", ["l2", "cosine", "inner_product"])
def test_ties_past_the_list(gpu, orc, monkeypatch, metric):
    """40 identical rows: each has 39 neighbours at one distance, more than K' = 26 list entries.  The 26th bound cannot lie
    above the tied distance, the strict certificate fails, and the gathered walk must itself leave the query's slot out."""
    dim, k = 33, 10
    X = np.concatenate([np.tile(gauss(1, dim, 3), (40, 1)), gauss(60, dim, 4)])
    ids = np.arange(1000, 1100, dtype=np.int64)
    c = Case(orc, metric, 0, X, ids)
    want = c.reference(k)
    for s in range(40):  # the other 39 in slot order, itself left out
        assert want[0][s].tolist() == [int(ids[t]) for t in range(40) if t != s][:k]
    g = make_index(gpu, c)
    for path in PATHS:
        with env(monkeypatch, path):
            got, st = knn(g, k)
        check(got, want, path)
        if not path:
            assert st["n_mfma_queries"] == 100 and st["n_fallback_queries"] >= 40, st
    g.close()


# ───────────────────────── 4. geometry ─────────────────────────

@pytest.mark.parametrize("metric", ["l2", "cosine", "inner_product"])
def test_geometry(gpu, orc, metric):
    dim, k = 33, 10
    for n in (1, 2, 5, 128, 129):
        c = Case(orc, metric, 0, gauss(n, dim, 70 + n), np.arange(1, n + 1, dtype=np.int64))
        g = make_index(gpu, c)
        got, st = knn(g, k)
        check(got, c.reference(k), n)
        assert (got[2] == min(k, n - 1)).all() and st["n_queries"] == n
        if n == 129:  # the last slot deleted: the last query tile holds one slot, and it is never emitted
            assert g.delete(129) == 0
            c.set_dead([128])
            got, st = knn(g, k)
            check(got, c.reference(k), "last slot deleted")
            assert got[2][128] == -1 and (got[0][128] == -1).all() and np.isinf(got[1][128]).all() and st["n_queries"] == 128
        if n == 5:  # every row deleted
            for i in range(1, 6):
                assert g.delete(i) == 0
            (gi, gd, gc), st = knn(g, k)
            assert (gc == -1).all() and (gi == -1).all() and np.isinf(gd).all() and st["n_queries"] == 0
            ids, nbr, ds, cnt = g.knn_graph(k)
            assert len(ids) == 0 and nbr.shape == (0, k) and ds.shape == (0, k) and len(cnt) == 0
        g.close()
    e = gpu.HnswIndex(dim, metric, 8, 40)  # never held a row
    gi, gd, gc = e.knn_graph_slots(k)
    assert gi.shape == (0, k) and gd.shape == (0, k) and gc.shape == (0,)
    assert all(len(a) == 0 for a in e.knn_edges(k))
    e.close()
    c = Case(orc, metric, 0, gauss(140, dim, 77), np.arange(1, 141, dtype=np.int64))  # k = 128 on 140 rows
    g = make_index(gpu, c)
    check(knn(g, 128)[0], c.reference(128), 128)
    for bad_k, r in ((0, None), (129, None), (10, float("nan"))):
        with pytest.raises(gpu.hnsw.MuninnHipError, match=r"^mn_hnsw_knn_graph:"):
            g.knn_graph_slots(bad_k, r)
    g.close()


# ───────────────────────── 5. the Python faces ─────────────────────────

def test_python_faces_and_untouched_index(gpu, orc):
    dim, metric, k, n = 128, "cosine", 10, 700
    c = Case(orc, metric, 0, gauss(n, dim, 51), np.arange(1, n + 1, dtype=np.int64), dead=[7, 600, 699])
    g = make_index(gpu, c)
    Q = gauss(20, dim, 52)
    before = g.search_batch(Q, 10, 64)
    r = np.float32(np.median(c.reference(k)[1][c.live, k - 1]))
    for rad in (None, r):
        wi, wd, wc = c.reference(k, INF if rad is None else rad)
        ids, nbr, ds, cnt = g.knn_graph(k, rad)  # the live rows in slot order
        assert np.array_equal(ids, c.ids[c.live])
        check((nbr, ds, cnt), (wi[c.live], wd[c.live], wc[c.live]), rad)
        src, dst, dist, rank = g.knn_edges(k, rad)  # knn_graph flattened, ordered by (slot of src, rank)
        assert len(src) == cnt.sum() and rank.dtype == np.int32
        at = 0
        for i in range(len(ids)):
            m = int(cnt[i])
            assert (src[at:at + m] == ids[i]).all() and rank[at:at + m].tolist() == list(range(m))
            assert np.array_equal(dst[at:at + m], nbr[i, :m]) and same_bits(dist[at:at + m], ds[i, :m])
            at += m
        di, dd, dc = g.dev_malloc(n * k * 8), g.dev_malloc(n * k * 4), g.dev_malloc(n * 4)  # the _dev call equals the host call
        g.knn_graph_dev(k, di, dd, dc, rad)
        assert g.last_exact()["kernel_ms"] > 0 and g.last_exact()["n_queries"] == len(c.live)
        gi, gd, gc = np.empty((n, k), np.int64), np.empty((n, k), np.float32), np.empty(n, np.int32)
        g.dev_download(gi, di)
        g.dev_download(gd, dd)
        g.dev_download(gc, dc)
        check((gi, gd, gc), g.knn_graph_slots(k, rad), "dev")
        check((gi, gd, gc), (wi, wd, wc), "dev vs reference")
        for p in (di, dd, dc):
            g.dev_free(p)
    after = g.search_batch(Q, 10, 64)  # the index and its graph are left as they were
    assert np.array_equal(before[0], after[0]) and same_bits(before[1], after[1]) and np.array_equal(before[2], after[2])
    g.close()
