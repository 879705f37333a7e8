"""mn_graph_from_edges (csrc/mn_csr_build.hip): the CSR pair built on the device from an edge list, read back through
mn_graph_export_csr and held against graph.csr_pair_from_edges, the numpy stable argsort every parity test here already
depends on.  Offsets and targets must be equal and weights equal as 64-bit words, under both implementations
(MN_CSR_BUILD=sort: per-list sorts binned by degree; MN_CSR_BUILD=radix, also the default: one stable radix sort) and
under bin limits that push short lists through the long paths.  Rows are shuffled wherever a shape allows it, so that the slot a row takes
in the fill step is not its place in the result."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROUTES = ["sort", "radix", "default"]
NAN_PAYLOAD = np.array([0x7FF80000DEADBEEF, 0xFFF0000000000001], np.uint64).view(np.float64)  # a quiet and a signalling NaN


def _by_degree(degrees, n=None, seed=0):
    """rows in shuffled order: node v is the source of degrees[v] rows, destinations uniform over the n nodes"""
    rng = np.random.default_rng(seed)
    n = n or len(degrees)
    src = np.repeat(np.arange(len(degrees)), degrees)
    rng.shuffle(src)
    dst = rng.integers(0, n, len(src))
    return n, src.astype(np.int32), dst.astype(np.int32), rng.random(len(src))


def _shapes():
    rng = np.random.default_rng(11)
    e = np.zeros(0, np.int32)
    sh = {
        "one_node_no_rows": (1, e, e, np.zeros(0)),
        "five_nodes_no_rows": (5, e, e, np.zeros(0)),
        "three_self_loops": (1, np.zeros(3, np.int32), np.zeros(3, np.int32), np.array([3.0, 1.0, 2.0])),
        "degrees_0_1_2_63_64_65": _by_degree([0, 1, 2, 63, 64, 65], seed=1),
        # the default bin limits are 64 (registers) and 8192 (LDS): one hub below, at and above each
        "hubs_at_default_limits": _by_degree([63, 64, 65, 8191, 8192, 8193], n=40, seed=2),
        # every degree from 0 to 200: with MN_CSR_SORT_WAVE=4 MN_CSR_SORT_LDS=16 degrees 5 .. 200 cross all three paths
        "every_degree_to_200": _by_degree(list(range(201)), seed=3),
        "contention_5000_into_one": (2, np.zeros(5000, np.int32), np.ones(5000, np.int32), rng.random(5000)),
        "same_pair_six_weights": (3, np.full(6, 2, np.int32), np.full(6, 1, np.int32), np.array([6.0, 1.0, 5.0, 2.0, 4.0, 3.0])),
        "n4097_e20000": (4097, rng.integers(0, 4097, 20000).astype(np.int32), rng.integers(0, 4097, 20000).astype(np.int32),
                         rng.random(20000)),
    }
    n, s, d, w = _by_degree([0, 7, 70, 300], n=9, seed=4)
    w[::5] = -0.0
    w[1::7] = np.inf
    w[2::7] = -np.inf
    w[3::11] = NAN_PAYLOAD[0]
    w[4::13] = NAN_PAYLOAD[1]
    sh["special_weights"] = (n, s, d, w)
    return sh


SHAPES = _shapes()
_expected = {}


def _want(name, weighted=True):
    """csr_pair_from_edges of a shape, computed once"""
    key = (name, weighted)
    if key not in _expected:
        import muninn_amd

        n, s, d, w = SHAPES[name]
        _expected[key] = muninn_amd.pkg.graph.csr_pair_from_edges(n, s, d, w if weighted else None)
    return _expected[key]


def _route(monkeypatch, route, wave=None, lds=None):
    for k, v in (("MN_CSR_BUILD", None if route == "default" else route), ("MN_CSR_SORT_WAVE", wave), ("MN_CSR_SORT_LDS", lds)):
        if v is None:
            monkeypatch.delenv(k, raising=False)
        else:
            monkeypatch.setenv(k, str(v))


def _same(got, off, tgt, w):
    assert got[0].dtype == np.int32 and got[1].dtype == np.int32
    assert np.array_equal(got[0], off)
    assert np.array_equal(got[1], tgt)
    if w is None:
        assert got[2] is None
    else:
        assert got[2] is not None and np.array_equal(got[2].view(np.uint64), w.view(np.uint64))


def _check(gpu, name, weighted=True, lists="both"):
    n, s, d, w = SHAPES[name]
    want = _want(name, weighted)
    g = gpu.graph.Graph.from_edges(n, s, d, w if weighted else None, lists=lists)
    try:
        zeros = np.zeros(n + 1, np.int32)
        if lists in ("both", "out"):
            _same(g.export_csr("out"), *want[0:3])
        else:
            assert np.array_equal(g.export_csr("out")[0], zeros) and len(g.export_csr("out")[1]) == 0
        if lists in ("both", "in"):
            _same(g.export_csr("in"), *want[3:6])
        else:
            assert np.array_equal(g.export_csr("in")[0], zeros) and len(g.export_csr("in")[1]) == 0
    finally:
        g.close()


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("name", sorted(SHAPES))
def test_device_csr_equals_host_csr(gpu, monkeypatch, name, route):
    _route(monkeypatch, route)
    _check(gpu, name)


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("name", ["every_degree_to_200", "hubs_at_default_limits", "degrees_0_1_2_63_64_65"])
def test_small_bin_limits_send_short_lists_through_every_path(gpu, monkeypatch, name, route):
    """limits 4 and 16: degrees 2 .. 4 sort in registers, 5 .. 16 in LDS, 17 and up in the segmented sort"""
    _route(monkeypatch, route, wave=4, lds=16)
    _check(gpu, name)


@pytest.mark.parametrize("wave,lds", [(0, 0), (64, 0), (0, 8192), (1, 2), (1000, 100000)])
def test_any_bin_limits_give_the_same_bytes(gpu, monkeypatch, wave, lds):
    """limits outside their range are clamped (64 and 8192 at most); a register limit above the LDS limit leaves the LDS
    bin empty; 0 sends everything to the next path"""
    _route(monkeypatch, "sort", wave=wave, lds=lds)
    _check(gpu, "every_degree_to_200")


@pytest.mark.parametrize("route", ROUTES)
def test_unweighted(gpu, monkeypatch, route):
    _route(monkeypatch, route)
    _check(gpu, "every_degree_to_200", weighted=False)
    _check(gpu, "five_nodes_no_rows", weighted=False)


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("lists", ["out", "in"])
def test_one_direction_only(gpu, monkeypatch, lists, route):
    _route(monkeypatch, route)
    _check(gpu, "degrees_0_1_2_63_64_65", lists=lists)
    _check(gpu, "n4097_e20000", lists=lists)


@pytest.mark.parametrize("route", ROUTES)
def test_two_successive_calls_give_identical_bytes(gpu, monkeypatch, route):
    _route(monkeypatch, route)
    n, s, d, w = SHAPES["hubs_at_default_limits"]
    runs = []
    for _ in range(2):
        g = gpu.graph.Graph.from_edges(n, s, d, w)
        runs.append([a.tobytes() for which in ("out", "in") for a in g.export_csr(which)])
        g.close()
    assert runs[0] == runs[1]


def test_bad_input_is_refused_with_a_message_and_the_process_goes_on(gpu, monkeypatch):
    """input checks: the index is compared on the device before anything is written through it"""
    G = gpu.graph.Graph
    for route in ROUTES:
        _route(monkeypatch, route)
        for bad_src, bad_dst in (([0, 1, 5, 2], [1, 2, 3, 4]), ([0, 1, 2, 3], [1, -1, 3, 4]), ([0, 1, 2, 2 ** 31 - 1], [1, 2, 3, 4])):
            with pytest.raises(gpu.MuninnHipError, match=r"row \d names node .* outside 0 \.\. 4"):
                G.from_edges(5, bad_src, bad_dst, [1.0, 2.0, 3.0, 4.0])
        with pytest.raises(gpu.MuninnHipError, match="row 2 names node 5 -> 3"):  # the first bad row, whichever lane saw it first
            G.from_edges(5, [0, 1, 5, 9], [1, 2, 3, 9])
        with pytest.raises(gpu.MuninnHipError, match="outside an empty graph"):
            G.from_edges(0, [0], [0])
        L = gpu.graph._glib()
        one = np.zeros(1, np.int32)
        assert L.mn_graph_from_edges(5, -1, one.ctypes.data, one.ctypes.data, None, 3, 0) is None
        assert b"negative row count -1" in L.mn_graph_last_error()
        assert L.mn_graph_from_edges(5, 2 ** 31 - 1, one.ctypes.data, one.ctypes.data, None, 3, 0) is None
        assert b"exceed int32 offsets" in L.mn_graph_last_error()
        assert L.mn_graph_from_edges(5, 1, one.ctypes.data, one.ctypes.data, None, 0, 0) is None
        assert b"bad arguments" in L.mn_graph_last_error()
        assert L.mn_graph_from_edges(-1, 0, None, None, None, 3, 0) is None
        _check(gpu, "degrees_0_1_2_63_64_65")
    empty = G.from_edges(0, [], [])
    assert len(empty.export_csr("out")[0]) == 1
    empty.close()


@pytest.mark.parametrize("route", ROUTES)
def test_the_built_graph_is_an_ordinary_handle(gpu, monkeypatch, route):
    """degree() and bfs() on it equal those on Graph(...) over the host CSR"""
    _route(monkeypatch, route)
    n, s, d, w = SHAPES["n4097_e20000"]
    a = gpu.graph.Graph.from_edges(n, s, d, w)
    b = gpu.graph.Graph(n, *_want("n4097_e20000"))
    try:
        for x, y in zip(a.degree(), b.degree()):
            assert np.array_equal(x.view(np.uint64), y.view(np.uint64))
        for direction in ("forward", "reverse", "both"):
            for x, y in zip(a.bfs(int(s[0]), 6, direction), b.bfs(int(s[0]), 6, direction)):
                assert np.array_equal(x, y)
        assert gpu.graph._glib().mn_graph_out_edge_count(a.h) == len(s)
    finally:
        a.close()
        b.close()


def test_retain_keeps_the_handle_until_the_last_owner_lets_go(gpu):
    n, s, d, w = SHAPES["same_pair_six_weights"]
    g = gpu.graph.Graph.from_edges(n, s, d, w)
    h, L = g.h, g.L
    L.mn_graph_retain(h)
    g.close()  # one of two owners
    off, tgt = np.zeros(n + 1, np.int32), np.zeros(6, np.int32)
    wv = np.zeros(6)
    assert L.mn_graph_export_csr(h, 1, off, tgt.ctypes.data, wv.ctypes.data) == 1
    assert off.tolist() == [0, 0, 6, 6] and tgt.tolist() == [2] * 6 and wv.tolist() == [6.0, 1.0, 5.0, 2.0, 4.0, 3.0]
    L.mn_graph_destroy(C.c_void_p(h))
