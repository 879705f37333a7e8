import numpy as np


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int32) if a.dtype == np.float32 else a


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


def gauss(n, d, seed):
    return np.random.default_rng(seed).standard_normal((n, d), dtype=np.float32)


def small_hnsw_table(c, name):
    """The smallest table on which a grouped cursor can go wrong: 40 rows of dim 8 under rowids 1..40 (slot = rowid - 1),
    l2, m = 4, then rowids 7 and 23 deleted.  Returns the vectors."""
    X = gauss(40, 8, 101)
    c.execute(f"CREATE VIRTUAL TABLE {name} USING hnsw_index(dimensions=8, metric='l2', m=4)")
    with c:
        for i in range(40):
            c.execute(f"INSERT INTO {name} (rowid, vector) VALUES (?, ?)", (i + 1, X[i].tobytes()))
        for gone in (7, 23):
            c.execute(f"DELETE FROM {name} WHERE rowid = ?", (gone,))
    return X


def ranks_within(groups):
    """0, 1, 2, ... restarting whenever the group changes: the rank of every row within its group, rows as they came."""
    out, last, r = [], object(), 0
    for g in groups:
        r = r + 1 if g == last else 0
        last = g
        out.append(r)
    return out


def recall_at_k(found, truth):
    hit = 0
    for f, t in zip(found, truth):
        hit += len(set(int(x) for x in f if x >= 0) & set(int(x) for x in t))
    return hit / float(truth.shape[0] * truth.shape[1])


def overgrown_case(mk, long_lists=True):
    """Index whose lists exceed M_max two ways: naturally (M = 2, 80 % deleted: the reconnection step,
    src/hnsw_algo.c:775-782, grows lists — node_add_neighbor has no bound) and, optionally, through the load API (lists
    of up to 3x M_max, as a database could hold them).  Then more inserts: every insert that touches such a list prunes
    ALL of it back to M_max (:601-646).  Returns the index and the ids for graph()."""
    n, d, M, efc = 1300, 2, 2, 3
    X = gauss(n, d, 31)
    ids = np.arange(1, n + 1, dtype=np.int64)
    x = mk(d, "l2", M, efc)
    assert x.insert_many(ids[:1000], X[:1000]) == 0
    for v in np.random.default_rng(4).permutation(ids[:1000])[:800]:
        assert x.delete(int(v)) == 0
    grown = x.graph(ids[:1000])
    if long_lists:
        rng = np.random.default_rng(6)
        live = [int(i) for i in ids[:1000] if x.node_deleted(int(i)) == 0]
        for i in live[::7]:
            for l in range(x.node_level(i) + 1):
                cand = [c for c in live if c != i and x.node_level(c) >= l]
                extra = rng.choice(cand, min(len(cand), 3 * (2 * M if l == 0 else M)), replace=False)
                assert x.load_neighbors(i, l, np.asarray(extra, np.int64)) == 0
    return x, ids, X, grown


def check_topk_f64(got, X, Q, ids, deleted, k, metric, c=4.0):
    """Rounding-aware comparison of a top-k id list with float64 distances.  eps bounds one pair's f32 error:
    c·dim·2⁻²⁴·(|q|²+|x|²) (l2), c·dim·2⁻²⁴ (cosine), c·dim·2⁻²⁴·|q||x| (inner product)."""
    X64, Q64 = X.astype(np.float64), Q.astype(np.float64)
    dim = X.shape[1]
    u = 2.0 ** -24
    qn, xn = np.linalg.norm(Q64, axis=1), np.linalg.norm(X64, axis=1)
    if metric == "l2":
        D = (qn ** 2)[:, None] + (xn ** 2)[None, :] - 2 * Q64 @ X64.T
        E = c * dim * u * ((qn ** 2)[:, None] + (xn ** 2)[None, :])
    elif metric == "cosine":
        D = 1 - (Q64 @ X64.T) / np.maximum(qn[:, None] * xn[None, :], 1e-300)
        E = np.full(D.shape, c * dim * u)
    else:
        D = -(Q64 @ X64.T)
        E = c * dim * u * (qn[:, None] * xn[None, :])
    live = np.ones(len(ids), bool)
    live[[int(np.searchsorted(ids, d)) for d in deleted]] = False
    n_live = int(live.sum())
    for i in range(len(Q)):
        row = got[i]
        kk = min(k, n_live)
        assert (row[kk:] == -1).all() and (row[:kk] >= 0).all(), (i, row)
        r = row[:kk]
        assert len(set(r.tolist())) == kk, (i, r)
        assert not np.isin(r, deleted).any(), (i, r)
        pos = np.searchsorted(ids, r)
        assert (ids[pos] == r).all(), (i, r)
        d, e = D[i], E[i]
        kth = np.sort(d[live])[kk - 1]
        assert (d[pos] <= kth + e[pos]).all(), (i, r, d[pos] - kth, e[pos])
        must = np.nonzero(live & (d < kth - e))[0]
        assert np.isin(must, pos).all(), (i, np.setdiff1d(must, pos))
        assert (d[pos][:-1] <= d[pos][1:] + e[pos][:-1] + e[pos][1:]).all(), (i, r)
