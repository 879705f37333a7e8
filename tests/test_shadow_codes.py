"""The 10-bit coded shadow (mn_device.hpp: three signed codes per dword, rows of whole 128-byte lines of 96 codes, the row's own
scale s = max|x| / 511) behind k_beam<LP>'s lower bound.  The bound only decides which candidates have their
f32 rows read, so every search must return what it returns with the filter off (MN_LOWPREC_FILTER=0, read per launch) and what
the CPU oracle returns on the same graph — at every way a coded row can end (on a line, in padding codes, after a short tail), on
rows that sit on the code's edges, and while still rejecting about as many candidates as the fp16 shadow it replaced did."""
import numpy as np
import pytest

from util import gauss, same_bits

pytestmark = pytest.mark.gpu

METRICS = ["l2", "cosine", "inner_product"]


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


def _check(gpu, orc, monkeypatch, X, Q, d, metric, tag, rejects):
    """filter on == filter off == the oracle loaded from the device, for ef in (10, 64)"""
    n = len(X)
    g = gpu.HnswIndex(d, metric, 8, 60)
    assert g.build(np.arange(1, n + 1, dtype=np.int64), X, 16, 8192) == 0
    o = orc.Oracle(d, metric, 8, 60)
    o.load_from_device(g, vectors=X)
    for ef in (10, 64):
        on, off = _search_both(g, Q, 10, ef, monkeypatch)
        _assert_same(on, off, (tag, metric, ef))
        wi, wd, wc = o.search_many(Q, 10, ef)
        assert np.array_equal(on[0][0], wi) and same_bits(on[0][1], wd), (tag, metric, ef)
        if rejects:
            assert on[1]["last_n_exact_rows"] < on[1]["last_n_dist"], (tag, metric, ef)
    g.close()


# 192, 768, 1536: the coded row ends on a line (2, 8, 16 lines); 256, 320, 512, 704, 1024: it ends in 32 or 64 padding codes
# (3, 4, 6, 8, 11 lines: the 8-, 2- and 1-line steps of lo_rows_accumulate in every combination); 255, 766: a zero tail inside ld
@pytest.mark.parametrize("dim", [192, 768, 1536, 256, 320, 512, 704, 1024, 255, 766])
@pytest.mark.parametrize("metric", METRICS)
def test_coded_rows_every_padding(gpu, orc, monkeypatch, metric, dim):
    n = 3000
    X = gauss(n, dim, 100 + dim)
    Q = np.concatenate([gauss(200, dim, 200 + dim), X[1000:1050]])
    _check(gpu, orc, monkeypatch, X, Q, dim, metric, dim, rejects=True)


def _edge_rows(n, d, seed):
    """a tenth of the rows each: see the comments; the rest gaussian.  Returns the rows and the first index of every kind that queries are drawn from."""
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, d), dtype=np.float32)
    k = n // 10
    sign = lambda shape: np.where(rng.random(shape) < 0.5, np.float32(-1), np.float32(1))
    # one element at ±max and the rest 1e-4 of it: codes ±511 and 0
    a = 0
    m = np.exp(rng.uniform(-3, 3, k)).astype(np.float32)
    X[a:a + k] = (np.float32(1e-4) * m)[:, None] * sign((k, d))
    X[np.arange(a, a + k), rng.integers(0, d, k)] = m * sign(k)
    # all elements of equal magnitude, random signs: every code is ±511
    a = k
    X[a:a + k] = np.exp(rng.uniform(-3, 3, k)).astype(np.float32)[:, None] * sign((k, d))
    # exact half-steps (j + 1/2) s: ties for rintf.  s = odd * 2^e and element 0 = 511 s are exact in f32, so fl32(max / 511) is s
    a = 2 * k
    s = (rng.choice([1, 3, 5, 7], k) * 2.0 ** rng.integers(-12, 4, k)).astype(np.float32)
    j = rng.integers(-511, 511, (k, d)).astype(np.float32)  # (j + 1/2) in [-510.5, 510.5]
    X[a:a + k] = (j + np.float32(0.5)) * s[:, None]
    X[a:a + k, 0] = np.float32(511) * s
    # the only large element is negative
    a = 3 * k
    X[a:a + k] = np.float32(0.01) * rng.standard_normal((k, d), dtype=np.float32)
    X[np.arange(a, a + k), rng.integers(0, d, k)] = np.float32(-5)
    # zero rows
    a = 4 * k
    X[a:a + k] = 0
    # rows scaled to 1e-38 (s subnormal), 1e-41 (subnormal elements) and 3e38 (|x| beyond the f32 range)
    a = 5 * k
    t = k // 3
    unit = X[a:a + k] / np.abs(X[a:a + k]).max(axis=1, keepdims=True)
    X[a:a + t] = unit[:t] * np.float32(1e-38)
    X[a + t:a + 2 * t] = unit[t:2 * t] * np.float32(1e-41)
    X[a + 2 * t:a + k] = unit[2 * t:] * np.float32(3e38)
    # 300 copies of one (gaussian) row: d == worst0 at the threshold
    a = 6 * k
    X[a:a + 300] = X[n - 1]
    # first row of every kind that can serve as a query too.  Not the 3e38 rows: a query whose f32 norm is infinite makes the
    # reference's own cosine distance inf / inf (and its dot products inf - inf), and the sign bit of that NaN is the host's or the
    # device's, not the search's — the rows stay in the database, where every query meets them
    kinds = [0, k, 2 * k, 3 * k, 4 * k, 5 * k, 5 * k + t, 6 * k, n - 10, n - 5]
    return X, kinds


@pytest.mark.parametrize("dim", [256, 768])
@pytest.mark.parametrize("metric", METRICS)
def test_code_edges(gpu, orc, monkeypatch, metric, dim):
    n = 3000
    X, kinds = _edge_rows(n, dim, 300 + dim)
    # 200 gaussian queries and 50 database rows: five of every kind (ten of the plain gaussian rows)
    Q = np.concatenate([gauss(200, dim, 400 + dim)] + [X[i:i + 5] for i in kinds])
    _check(gpu, orc, monkeypatch, X, Q, dim, metric, "edges", rejects=False)


# k_beam<LP> with the fp16 shadow (commit 419fe81, "Split mn_graph.hip by algorithm ..."), this very index and these queries:
# last_n_exact_rows / last_n_dist, measured on an MI355X in the same run as the coded shadow's first ratio
# (profiles/r07_coded_shadow.txt, "rejection power")
PARENT_EXACT_ROWS = 343_561
PARENT_N_DIST = 1_940_069


def test_rejection_power_20k_x_768(gpu):
    """A bound that silently stopped rejecting — a wrong resid, field or scale — would still return the right answers.  The
    coded shadow may let at most 1.15 x the fp16 shadow's share of the candidates through to the exact walk (the CPU model of
    scripts/shadow_code_model.py predicts 1.06 x)."""
    n, d, nq = 20_000, 768, 500
    X = gauss(n, d, 42)
    Q = gauss(nq, d, 43)
    g = gpu.HnswIndex(d, "cosine", 16, 100)
    assert g.build(np.arange(1, n + 1, dtype=np.int64), X, 16, 8192) == 0
    g.search_batch(Q, 10, 128)
    st = g.last_launch()
    g.close()
    ratio = st["last_n_exact_rows"] / st["last_n_dist"]
    parent = PARENT_EXACT_ROWS / PARENT_N_DIST
    print(f"exact rows {st['last_n_exact_rows']} of n_dist {st['last_n_dist']}: ratio {ratio:.5f}; parent {parent:.5f}; "
          f"{ratio / parent:.4f} x")
    assert st["last_n_dist"] == PARENT_N_DIST  # the same searches
    assert ratio <= 1.15 * parent, (ratio, parent)
