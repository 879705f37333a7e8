"""The exact walk of the fp16 filter's survivors (k_beam<LP>, sse_rows_spread) spreads a row over 4, 8 or 16
lanes by the number of survivors of a pass; MN_SURVIVOR_LANES=4|8|16 (read per launch) forces one layout.  Every layout adds the
reference's terms in the reference's order, so every search must return what it returns with the filter off and what the CPU
oracle returns — ids, distance bits, counts and counters — at every row length the shadow is kept for, and no case may pass
without its layout having run (last_n_rows_lanes4 / 8 / 16)."""
import numpy as np
import pytest

from test_lowprec_filter import _adversarial_rows
from util import gauss, same_bits

pytestmark = pytest.mark.gpu

METRICS = ["l2", "cosine", "inner_product"]
# whole lines of fp16 (ld = dim), and dim = ld - 1, ld - 2: 15 and 47 quad blocks, chain positions past them and a scalar tail
LENGTHS = [192, 256, 320, 448, 768, 1024, 1536, 255, 766]
LAYOUTS = [None, 4, 8, 16]


def _launch(g, Q, k, ef, monkeypatch, lanes=None, filter_off=False):
    monkeypatch.delenv("MN_LOWPREC_FILTER", raising=False)
    monkeypatch.delenv("MN_SURVIVOR_LANES", raising=False)
    if filter_off:
        monkeypatch.setenv("MN_LOWPREC_FILTER", "0")
    if lanes is not None:
        monkeypatch.setenv("MN_SURVIVOR_LANES", str(lanes))
    r = g.search_batch(Q, k, ef)
    st = g.last_launch()
    monkeypatch.delenv("MN_LOWPREC_FILTER", raising=False)
    monkeypatch.delenv("MN_SURVIVOR_LANES", raising=False)
    return r, st


def _check_layouts(g, o, Q, k, ef, monkeypatch, tag, all_three_in_auto=False, must_filter=True):
    (wi, wd, wc), sw = _launch(g, Q, k, ef, monkeypatch, filter_off=True)
    assert sw["last_n_exact_rows"] == sw["last_n_dist"], tag
    assert (sw["last_n_rows_lanes4"], sw["last_n_rows_lanes8"], sw["last_n_rows_lanes16"]) == (sw["last_n_dist"], 0, 0), tag
    oi, od, oc = o.search_many(Q, k, ef)
    assert np.array_equal(wi, oi) and same_bits(wd, od) and np.array_equal(wc, oc), tag
    exact_rows = None
    for lanes in LAYOUTS:
        t = tag + (lanes,)
        (gi, gd, gc), st = _launch(g, Q, k, ef, monkeypatch, lanes=lanes)
        assert np.array_equal(gc, wc), t
        assert np.array_equal(gi, wi), t
        assert same_bits(gd, wd), t
        assert np.array_equal(gi, oi) and same_bits(gd, od), t
        assert (st["last_n_dist"], st["last_n_expanded"]) == (sw["last_n_dist"], sw["last_n_expanded"]), t
        if exact_rows is None:
            exact_rows = st["last_n_exact_rows"]
        assert st["last_n_exact_rows"] == exact_rows, t  # the bound does not depend on the layout
        if must_filter:
            assert 0 < exact_rows < st["last_n_dist"], t
        l4, l8, l16 = st["last_n_rows_lanes4"], st["last_n_rows_lanes8"], st["last_n_rows_lanes16"]
        assert l4 + l8 + l16 == exact_rows and min(l4, l8, l16) >= 0, t
        # the rows of the greedy descent and of the entry point are always walked by 4 lanes; the layer-0 passes by the layout
        if lanes == 4:
            assert (l4, l8, l16) == (exact_rows, 0, 0), t
        elif lanes == 8:
            assert l8 > 0 and l16 == 0, t
        elif lanes == 16:
            assert l16 > 0 and l8 == 0, t
        elif all_three_in_auto:
            assert l4 > 0 and l8 > 0 and l16 > 0, t
        else:
            assert l8 + l16 > 0, t


@pytest.mark.parametrize("dim", LENGTHS)
@pytest.mark.parametrize("metric", METRICS)
def test_layouts_equal_filter_off_and_oracle(gpu, orc, monkeypatch, metric, dim):
    n, nq, ef = 20_000, 300, 64
    X = gauss(n, dim, 100 + dim)
    Q = gauss(nq, dim, 200 + dim)
    g = gpu.HnswIndex(dim, metric, 8, 60)  # (the reference's summation order is the default)
    assert g.build(np.arange(1, n + 1, dtype=np.int64), X, 16, 8192) == 0
    o = orc.Oracle(dim, metric, 8, 60)
    o.load_from_device(g, vectors=X)
    _check_layouts(g, o, Q, 10, ef, monkeypatch, (metric, dim, ef), all_three_in_auto=(dim == 768))
    g.close()


@pytest.mark.parametrize("dim", [256, 768])
@pytest.mark.parametrize("metric", METRICS)
def test_layouts_on_adversarial_rows(gpu, orc, monkeypatch, metric, dim):
    """huge and tiny elements in one row, subnormals, zero rows, rows near the f32 range, duplicates, queries equal to rows"""
    n = 3000
    X = _adversarial_rows(n, dim, 7)
    X[2000:2300] = X[1500]
    g = gpu.HnswIndex(dim, metric, 8, 60)
    assert g.build(np.arange(1, n + 1, dtype=np.int64), X, 16, 8192) == 0
    Q = np.concatenate([X[1490:1600], X[:60], gauss(150, dim, 11)])
    o = orc.Oracle(dim, metric, 8, 60)
    o.load_from_device(g, vectors=X)
    for ef in (10, 40, 128):
        _check_layouts(g, o, Q, 10, ef, monkeypatch, (metric, dim, ef), must_filter=False)
    g.close()
