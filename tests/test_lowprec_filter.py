"""The fp16 shadow's lower bound (k_beam<LP>) only decides which candidates have their f32 rows read: every
search must return exactly what it returns with the filter off (MN_LOWPREC_FILTER=0, read per launch) — ids, distance bits,
counts, and the n_dist / n_expanded counters."""
import importlib.util
import os

import numpy as np
import pytest

from util import gauss, same_bits

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
METRICS = ["l2", "cosine", "inner_product"]


def _bench():
    spec = importlib.util.spec_from_file_location("_bench_gen", os.path.join(ROOT, "bench.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def _search_both(g, Q, k, ef, monkeypatch):
    """(results, counters) with the filter on, then off"""
    out = []
    for off in (False, True):
        if off:
            monkeypatch.setenv("MN_LOWPREC_FILTER", "0")
        else:
            monkeypatch.delenv("MN_LOWPREC_FILTER", raising=False)
        r = g.search_batch(Q, k, ef)
        out.append((r, g.last_launch()))
    monkeypatch.delenv("MN_LOWPREC_FILTER", raising=False)
    return out


def _assert_same(on, off, tag):
    (gi, gd, gc), st = on
    (wi, wd, wc), sw = off
    assert np.array_equal(gc, wc), tag
    assert np.array_equal(gi, wi), tag
    assert same_bits(gd, wd), tag
    assert (st["last_n_dist"], st["last_n_expanded"]) == (sw["last_n_dist"], sw["last_n_expanded"]), tag
    assert sw["last_n_exact_rows"] == sw["last_n_dist"], tag
    assert st["last_n_exact_rows"] <= st["last_n_dist"], tag


@pytest.mark.parametrize("dataset", ["gaussian", "lowrank16", "clustered0.01"])
@pytest.mark.parametrize("metric", METRICS)
def test_filter_on_equals_off_100k_x_768(gpu, monkeypatch, dataset, metric):
    b = _bench()
    n, d, nq = 100_000, 768, 2000
    X = b.gen_vectors(n, d, 42, dataset)
    Q = b.gen_vectors(nq, d, 43, dataset)
    orders = ["sse", "wave"] if dataset == "gaussian" else ["sse"]
    for order in orders:
        g = gpu.HnswIndex(d, metric, 16, 100, order=gpu.ORDER_SSE if order == "sse" else gpu.ORDER_WAVE)
        assert g.build(np.arange(1, n + 1, dtype=np.int64), X, 16, 8192) == 0
        for ef in (64, 128, 256):
            on, off = _search_both(g, Q, 10, ef, monkeypatch)
            _assert_same(on, off, (dataset, metric, order, ef))
            assert on[1]["last_n_exact_rows"] < on[1]["last_n_dist"], (dataset, metric, order, ef)
        g.close()


def _adversarial_rows(n, d, seed):
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, d), dtype=np.float32)
    k = n // 10
    # rows mixing huge and tiny elements, subnormals, all-zero rows, rows near the f32 range
    mix = rng.standard_normal((k, d), dtype=np.float32)
    mix[:, ::3] *= np.float32(1e30)
    mix[:, 1::3] *= np.float32(1e-30)
    X[:k] = mix
    X[k:k + 20] = 0.0
    X[k + 20:k + 40] = rng.standard_normal((20, d), dtype=np.float32) * np.float32(1e-41)  # subnormal
    X[k + 40:k + 60, : d // 2] = np.float32(3e38)
    X[k + 60:k + 80, 5] = np.float32(1e-38)
    return X


@pytest.mark.parametrize("metric", METRICS)
def test_adversarial_rows_against_filter_off_and_oracle(gpu, orc, monkeypatch, metric):
    n, d = 3000, 256
    X = _adversarial_rows(n, d, 7)
    # duplicates of one vector, and queries equal to database vectors: d == worst ties at the threshold
    X[2000:2300] = X[1500]
    ids = np.arange(1, n + 1, dtype=np.int64)
    g = gpu.HnswIndex(d, metric, 8, 60)
    assert g.build(ids, X, 16, 8192) == 0
    Q = np.concatenate([X[1490:1600], X[:60], gauss(150, d, 11)])
    o = orc.Oracle(d, metric, 8, 60)
    o.load_from_device(g, vectors=X)
    for ef in (10, 40, 128):
        on, off = _search_both(g, Q, 10, ef, monkeypatch)
        _assert_same(on, off, (metric, ef))
        wi, wd, wc = o.search_many(Q, 10, ef)
        assert np.array_equal(on[0][0], wi) and same_bits(on[0][1], wd), (metric, ef)
    g.close()


@pytest.mark.parametrize("metric", METRICS)
def test_rows_whose_squares_underflow(gpu, orc, monkeypatch, metric):
    """Rows of norm 1e-23 .. 1e-19: their elements' squares fall below the f32 normal range, so the row's f32 norm is well
    below |x|² — the cosine bound must rest on the stored norm itself.  Clustered, so that the queries' near neighbours are
    such rows and the worst result sits within a few hundredths of them."""
    n, d = 3000, 768
    rng = np.random.default_rng(17)
    C = rng.standard_normal((40, d), dtype=np.float32)
    X = C[rng.integers(0, 40, n)] + np.float32(0.05) * rng.standard_normal((n, d), dtype=np.float32)
    tiny = rng.random(n) < 0.6
    X[tiny] *= (10.0 ** rng.uniform(-24.5, -20.5, tiny.sum())).astype(np.float32)[:, None]
    Q = C[rng.integers(0, 40, 300)] + np.float32(0.05) * rng.standard_normal((300, d), dtype=np.float32)
    g = gpu.HnswIndex(d, metric, 8, 60)
    assert g.build(np.arange(1, n + 1, dtype=np.int64), X, 16, 8192) == 0
    o = orc.Oracle(d, metric, 8, 60)
    o.load_from_device(g, vectors=X)
    for ef in (10, 40, 128):
        on, off = _search_both(g, Q, 10, ef, monkeypatch)
        _assert_same(on, off, (metric, ef))
        wi, wd, wc = o.search_many(Q, 10, ef)
        assert np.array_equal(on[0][0], wi) and same_bits(on[0][1], wd), (metric, ef)
    g.close()


@pytest.mark.parametrize("metric", METRICS)
def test_non_finite_rows(gpu, monkeypatch, metric):
    n, d = 2000, 192
    X = gauss(n, d, 3)
    X[100:110, 7] = np.inf
    X[200:210, 9] = -np.inf
    X[300:310, 11] = np.nan
    g = gpu.HnswIndex(d, metric, 8, 60)
    assert g.build(np.arange(1, n + 1, dtype=np.int64), X, 16, 8192) == 0
    Q = np.concatenate([gauss(200, d, 4), X[95:115]])
    for ef in (20, 64):
        on, off = _search_both(g, Q, 10, ef, monkeypatch)
        _assert_same(on, off, (metric, ef))
    g.close()


def test_inserts_after_build_and_deletes(gpu, orc, monkeypatch):
    """inserts that make d_vectors (and the shadow with it) reallocate, then deletes: the shadow follows every row"""
    n0, n1, d = 1500, 6000, 320
    X = gauss(n1, d, 21)
    ids = np.arange(1, n1 + 1, dtype=np.int64)
    g = gpu.HnswIndex(d, "cosine", 8, 60)
    assert g.build(ids[:n0], X[:n0], 16, 8192) == 0
    for a in range(n0, n1, 1500):
        assert g.insert_batch(ids[a:a + 1500], X[a:a + 1500], gpu.BUILD_BATCHED) == 0
    assert g.insert(n1 + 1, X[17] * np.float32(3.0)) == 0  # one-row insert: the pinned single-row upload path
    Q = gauss(300, d, 22)
    on, off = _search_both(g, Q, 10, 64, monkeypatch)
    _assert_same(on, off, "inserts")
    assert on[1]["last_n_exact_rows"] < on[1]["last_n_dist"]
    for v in np.random.default_rng(5).permutation(ids[:n1])[:400]:
        assert g.delete(int(v)) == 0
    on, off = _search_both(g, Q, 10, 64, monkeypatch)
    _assert_same(on, off, "deletes")
    g.close()


def test_one_batch_1m_x_768(gpu, monkeypatch):
    b = _bench()
    n, d = 1_000_000, 768
    g = gpu.HnswIndex(d, "cosine", 16, 200)
    rc, _ = b.build_streamed(g, n, d, 42, "gaussian")
    assert rc == 0
    Q = b.gen_vectors(300, d, 43, "gaussian")
    on, off = _search_both(g, Q, 10, 128, monkeypatch)
    _assert_same(on, off, "1M")
    assert on[1]["last_n_exact_rows"] < on[1]["last_n_dist"]
    g.close()
