"""Exact k-NN search (mn_hnsw_search_exact_batch, csrc/mn_exact.hip) against the CPU oracle's distances, bit for bit.

Contract: over the live (and, with an allow-list, allowed) slots, d = the index's own distance (oracle.orc.dist_batch in the
index's order gives its bits); the answer is the k smallest under (d, slot); past counts[q] ids are -1 and distances +inf.
Three paths must give that one answer: the default (matrix-core candidate pass, re-score, certificate), MN_EXACT=valu (the
index's inner loop over every row) and MN_EXACT_SLACK=0 (lists without surplus: certificates fail, queries fall back)."""
import numpy as np
import pytest

from util import gauss, same_bits

pytestmark = pytest.mark.gpu

N, NQ = 2300, 140  # three row chunks of 768 rows (ex_chunks), the last ending in a ragged 128-row tile; two query tiles, the second ragged
KS = (1, 10, 32, 33, 128)  # 32 / 33: the last k the matrix-core pass serves and the first it does not
CONFIGS = [(m, d, o) for m in ("l2", "cosine", "inner_product") for d, o in
           ((4, 0), (33, 0), (128, 0), (128, 1), (200, 0), (768, 0), (768, 1))]
PATHS = ({}, {"MN_EXACT": "valu"}, {"MN_EXACT_SLACK": "0"})


def distances(orc, metric, order, X, Q):
    """[nq][n] the oracle's distance of every query to every row, in the index's order"""
    return np.stack([orc.dist_batch(metric, q, X, order) for q in Q])


def reference(orc, metric, order, X, ids, live, Q, k, D=None):
    """(ids [nq][k], dists [nq][k], counts [nq]) from the oracle's distances over the slots in `live` (ascending).
    D: distances(orc, metric, order, X, Q) where a caller ranks the same pairs more than once (a row's distance does not depend
    on the other rows of the call)."""
    nq = len(Q)
    ri = np.full((nq, k), -1, np.int64)
    rd = np.full((nq, k), np.inf, np.float32)
    rc = np.full(nq, min(k, len(live)), np.int32)
    if len(live) == 0:
        return ri, rd, rc
    Xl = np.ascontiguousarray(X[live]) if D is None else None
    for i in range(nq):
        d = orc.dist_batch(metric, Q[i], Xl, order) if D is None else D[i][live]
        o = np.lexsort((live, d))[:k]
        ri[i, :len(o)] = ids[live[o]]
        rd[i, :len(o)] = d[o]
    return ri, rd, rc


def exact(g, Q, k, allow=None):
    """search_exact_batch + the free check of the bound's derivation: no re-scored row lies below its bound"""
    out = g.search_exact_batch(Q, k, allow)
    st = g.last_exact()
    assert st["n_bound_violations"] == 0, st
    assert st["n_queries"] == len(Q)
    return out, st


def check(got, want, what):
    (gi, gd, gc), (wi, wd, wc) = got, want
    assert np.array_equal(gc, wc), what
    assert np.array_equal(gi, wi), (what, np.nonzero((gi != wi).any(axis=1))[0][:8])
    assert same_bits(gd, wd), what


def make_index(gpu, metric, order, X, ids, deleted=()):
    g = gpu.HnswIndex(X.shape[1], metric, 8, 40, order=order)
    assert g.insert_batch(ids, X, gpu.BUILD_BATCHED) == 0
    for d in deleted:
        assert g.delete(int(d)) == 0
    return g


@pytest.mark.parametrize("metric,dim,order", CONFIGS)
def test_three_paths_one_answer(gpu, orc, monkeypatch, metric, dim, order):
    X = gauss(N, dim, 21)
    X[17] = X[3]  # exact duplicate rows: the lower slot comes first
    Q = gauss(NQ, dim, 22)
    Q[0] = X[3]
    ids = np.arange(100, 100 + N, dtype=np.int64)
    top1 = int(np.argmin(orc.dist_batch(metric, Q[1], X, order)))  # a would-be top-1 goes
    dead = sorted({top1, 5, 1040} - {3, 17})
    g = make_index(gpu, metric, order, X, ids, ids[dead])
    live = np.setdiff1d(np.arange(N), dead)
    for k in KS:
        want = reference(orc, metric, order, X, ids, live, Q, k)
        assert top1 in (3, 17) or ids[top1] not in want[0]
        assert k == 1 or metric == "inner_product" or list(want[0][0][:2]) == [103, 117]
        for env in PATHS:
            for name, v in env.items():
                monkeypatch.setenv(name, v)
            got, st = exact(g, Q, k)
            for name in env:
                monkeypatch.delenv(name)
            check(got, want, (k, env))
            if "MN_EXACT" in env or k > 32:
                assert st["n_mfma_queries"] == 0 and st["n_fallback_queries"] == 0, (k, env, st)
            elif "MN_EXACT_SLACK" in env:
                assert st["n_mfma_queries"] == NQ and st["n_fallback_queries"] > 0, (k, env, st)
            else:
                # plain Gaussian rows: the gap between the k-th and the (k+16)-th distance is at least 6.6 bound widths of
                # 16 dim 2^-24 scale at dim 768 and over 50 at dim <= 200 — a sound bound of ordinary width certifies them
                assert st["n_mfma_queries"] == NQ and st["n_fallback_queries"] <= 0.05 * NQ, (k, st)
                assert st["n_rescored_rows"] == NQ * (k + 16), (k, st)
    # one query through the single-query call
    wi, wd, _ = reference(orc, metric, order, X, ids, live, Q[7:8], 10)
    gi, gd = g.search_exact(Q[7], 10)
    assert np.array_equal(gi, wi[0]) and same_bits(gd, wd[0])
    g.close()


@pytest.mark.parametrize("metric", ["l2", "cosine", "inner_product"])
def test_fewer_live_rows_than_k_and_an_emptied_index(gpu, orc, metric):
    dim, n = 33, 20
    X, Q = gauss(n, dim, 5), gauss(3, dim, 6)
    ids = np.arange(1, n + 1, dtype=np.int64)
    g = make_index(gpu, metric, 0, X, ids, [4, 9])
    live = np.setdiff1d(np.arange(n), [3, 8])
    for k in (18, 19, 32, 128):
        got, _ = exact(g, Q, k)
        check(got, reference(orc, metric, 0, X, ids, live, Q, k), k)
        assert (got[2] == min(k, 18)).all() and (got[0][:, 18:] == -1).all() and np.isinf(got[1][:, 18:]).all()
    for i in ids:
        if i not in (4, 9):
            assert g.delete(int(i)) == 0
    for k in (1, 10, 128):
        (gi, gd, gc), _ = exact(g, Q, k)
        assert (gc == 0).all() and (gi == -1).all() and np.isinf(gd).all()
    g.close()
    e = gpu.HnswIndex(dim, metric, 8, 40)  # never held a row
    (gi, gd, gc), _ = exact(e, Q, 5)
    assert (gc == 0).all() and (gi == -1).all() and np.isinf(gd).all()
    e.close()


@pytest.mark.parametrize("metric", ["l2", "cosine", "inner_product"])
def test_ties_at_the_kth_place_resolve_by_slot(gpu, orc, monkeypatch, metric):
    """Coordinates from {-1, 0, 1}: hundreds of rows share the k-th distance, the lower slots win.  The strict certificate
    (e_k < cut) cannot hold when rows outside the list may tie with the k-th, so these queries take the full walk."""
    rng = np.random.default_rng(9)
    X = rng.integers(-1, 2, (3000, 8)).astype(np.float32)
    X[(X == 0).all(axis=1)] = 1.0
    Q = rng.integers(-1, 2, (20, 8)).astype(np.float32)
    Q[(Q == 0).all(axis=1)] = 1.0
    ids = np.arange(1, 3001, dtype=np.int64)
    g = make_index(gpu, metric, 0, X, ids)
    live = np.arange(3000)
    for k in (10, 32):
        want = reference(orc, metric, 0, X, ids, live, Q, k)
        for env in PATHS:
            for name, v in env.items():
                monkeypatch.setenv(name, v)
            got, st = exact(g, Q, k)
            for name in env:
                monkeypatch.delenv(name)
            check(got, want, (k, env))
            if not env and metric != "cosine":
                assert st["n_fallback_queries"] > 0, st
    g.close()


def test_identical_rows(gpu, orc):
    X = np.tile(gauss(1, 16, 3), (500, 1))
    Q = gauss(4, 16, 4)
    ids = np.arange(1000, 1500, dtype=np.int64)
    for metric in ("l2", "cosine", "inner_product"):
        g = make_index(gpu, metric, 0, X, ids)
        for k in (10, 128):
            got, st = exact(g, Q, k)
            check(got, reference(orc, metric, 0, X, ids, np.arange(500), Q, k), (metric, k))
            assert (got[0] == ids[:k]).all()
            assert k > 32 or st["n_fallback_queries"] == len(Q)
        g.close()


@pytest.mark.parametrize("metric,order", [("l2", 0), ("cosine", 0), ("inner_product", 0), ("cosine", 1)])
def test_near_ties_where_approximate_and_exact_order_disagree(gpu, orc, metric, order):
    """20 Gaussian rows, 100 copies of each with one element moved by 1-3 ulps: the matrix cores' order of these rows is not
    the reference's, the bound still lies below every exact distance and the answer is the reference's."""
    dim = 768
    B = gauss(20, dim, 31)
    rng = np.random.default_rng(32)
    X = np.repeat(B, 100, axis=0)
    for r in range(len(X)):
        e = int(rng.integers(dim))
        for _ in range(int(rng.integers(1, 4))):
            X[r, e] = np.nextafter(X[r, e], np.float32(np.inf if r & 1 else -np.inf))
    ids = np.arange(1, len(X) + 1, dtype=np.int64)
    g = make_index(gpu, metric, order, X, ids)
    for k in (10, 32):
        got, _ = exact(g, B, k)
        check(got, reference(orc, metric, order, X, ids, np.arange(len(X)), B, k), k)
    g.close()


def test_allow_list_and_untouched_index(gpu, orc, monkeypatch):
    dim, metric = 128, "cosine"
    X, Q = gauss(N, dim, 41), gauss(NQ, dim, 42)
    ids = np.arange(100, 100 + N, dtype=np.int64)
    dead = [7, 600, 2299]
    g = make_index(gpu, metric, 0, X, ids, ids[dead])
    before = g.search_batch(Q, 10, 64)
    live = np.setdiff1d(np.arange(N), dead)
    rng = np.random.default_rng(43)
    pick = np.sort(rng.choice(N, N // 3, replace=False))
    allow = np.concatenate([ids[pick], ids[[7, 600]], [5, 10 ** 12]]).astype(np.int64)  # + two deleted, two never held
    rng.shuffle(allow)
    ok = np.setdiff1d(pick, dead)
    for k in (10, 33):
        want = reference(orc, metric, 0, X, ids, ok, Q, k)
        for env in PATHS:
            for name, v in env.items():
                monkeypatch.setenv(name, v)
            got, _ = exact(g, Q, k, allow)
            for name in env:
                monkeypatch.delenv(name)
            check(got, want, (k, env))
        (gi, gd, gc), _ = exact(g, Q, k, np.zeros(0, np.int64))
        assert (gc == 0).all() and (gi == -1).all() and np.isinf(gd).all()
        check(exact(g, Q, k, None)[0], reference(orc, metric, 0, X, ids, live, Q, k), k)
    few = ids[[11, 12, 13]]  # fewer allowed rows than k
    got, _ = exact(g, Q, 10, few)
    check(got, reference(orc, metric, 0, X, ids, np.array([11, 12, 13]), Q, 10), "few")
    after = g.search_batch(Q, 10, 64)
    assert np.array_equal(before[0], after[0]) and same_bits(before[1], after[1]) and np.array_equal(before[2], after[2])
    with pytest.raises(gpu.hnsw.MuninnHipError):
        g.search_exact_batch(Q, 129)
    with pytest.raises(gpu.hnsw.MuninnHipError):
        g.search_exact_batch(Q, 0)
    g.close()


def test_device_buffers(gpu, orc):
    dim, metric, k = 200, "l2", 10
    X, Q = gauss(700, dim, 51), gauss(9, dim, 52)
    ids = np.arange(1, 701, dtype=np.int64)
    g = make_index(gpu, metric, 0, X, ids)
    dq, di, dd, dc = g.dev_malloc(Q.nbytes), g.dev_malloc(9 * k * 8), g.dev_malloc(9 * k * 4), g.dev_malloc(9 * 4)
    g.dev_upload(dq, Q)
    g.search_exact_batch_dev(dq, 9, k, di, dd, dc)
    gi, gd, gc = np.empty((9, k), np.int64), np.empty((9, k), np.float32), np.empty(9, np.int32)
    g.dev_download(gi, di)
    g.dev_download(gd, dd)
    g.dev_download(gc, dc)
    check((gi, gd, gc), reference(orc, metric, 0, X, ids, np.arange(700), Q, k), "dev")
    assert g.last_exact()["n_bound_violations"] == 0 and g.last_exact()["kernel_ms"] > 0
    for p in (dq, di, dd, dc):
        g.dev_free(p)
    g.close()
