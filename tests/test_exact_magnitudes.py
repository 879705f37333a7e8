"""Exact k-NN search where the bound's derivation has cases, and where its lists and tiles have edges.

test_exact_search.py draws unit-scale rows; here the same contract — the k nearest live rows under (d, slot), ids and distances equal
to oracle.orc.dist_batch bit for bit, on the default path, under MN_EXACT=valu and under MN_EXACT_SLACK=0 — is held at scaled,
mixed-scale, non-centred, tiny, zero, huge and overflowing rows and queries, and at the list and tile geometry the launchers pick
from k, the slack, nq and n_slots.  A lower bound that is too high in one of these regimes drops a true neighbour silently:
n_bound_violations sees only the rows that made it into a list, the comparison with the oracle sees the answer.

Every family asserts first that the oracle's own distances hold no NaN: the contract orders "as floats", and a NaN's sign differs
between host and device (the note in test_shadow_codes.py).  Should a change of seed ever produce one, lower the magnitude."""
import numpy as np
import pytest

from test_exact_search import PATHS, check, distances, exact, make_index, reference
from util import bits, gauss, same_bits

pytestmark = pytest.mark.gpu

N, NQ = 1100, 130  # two row chunks, the second ending in a ragged tile; two query tiles, the second holding 2 queries
KS = (10, 32)
METRICS = ("l2", "cosine", "inner_product")
CONFIGS = [(m, d, 0) for m in METRICS for d in (33, 768)] + [("cosine", 768, 1)]
IDS = np.arange(100, 100 + N, dtype=np.int64)
NEG_ZERO = np.float32(-0.0).view(np.int32)


def base(dim):
    return gauss(N, dim, 1), gauss(NQ, dim, 2)


def all_distances(orc, metric, order, X, Q):
    """[nq][n] oracle distances; no NaN among them"""
    D = distances(orc, metric, order, X, Q)
    assert not np.isnan(D).any(), "the oracle's distances hold a NaN: lower the magnitude"
    return D


def three_paths(g, orc, monkeypatch, metric, order, X, ids, live, Q, D, what, ks=KS):
    """All three PATHS at every k against the oracle.  {k: (want, stats of the default path, [what each path gave])}"""
    out = {}
    for k in ks:
        want = reference(orc, metric, order, X, ids, live, Q, k, D)
        gots = []
        for env in PATHS:
            for name, v in env.items():
                monkeypatch.setenv(name, v)
            got, st = exact(g, Q, k)
            for name in env:
                monkeypatch.delenv(name)
            check(got, want, (what, metric, order, k, env))
            gots.append(got)
            mfma = "MN_EXACT" not in env and k <= 32
            assert st["n_mfma_queries"] == (len(Q) if mfma else 0), (what, k, env, st)
            if not mfma:
                assert st["n_fallback_queries"] == 0, (what, k, env, st)
            elif "MN_EXACT_SLACK" in env:
                # K' = k: cut = the largest bound of the list <= the largest distance of the list = e_k, so e_k < cut never holds;
                # every query falls back unless the list is short of k, which only fewer than k live rows make it
                assert st["n_fallback_queries"] == (len(Q) if len(live) >= k else 0), (what, k, env, st)
            if not env:
                out[k] = (want, st, gots)
                print(what, metric, order, X.shape[1], "k", k, "mfma", st["n_mfma_queries"], "fallback", st["n_fallback_queries"])
    return out


def whole_family(gpu, orc, monkeypatch, metric, order, X, Q, what, dead=(7, 600, 1099), D=None):
    """One index of N rows, three deleted; every k of KS on every path.  D: all_distances of the same arguments, if at hand."""
    D = all_distances(orc, metric, order, X, Q) if D is None else D
    g = make_index(gpu, metric, order, X, IDS, IDS[list(dead)])
    live = np.setdiff1d(np.arange(N), dead)
    out = three_paths(g, orc, monkeypatch, metric, order, X, IDS, live, Q, D, what)
    g.close()
    return out


# ───────────────────────── 1. scaled ─────────────────────────

@pytest.fixture(scope="module")
def unscaled(gpu, orc):
    """(metric, dim, order) -> whole_family of the base rows as they are, computed once per configuration"""
    done = {}

    def get(metric, dim, order):
        if (metric, dim, order) not in done:
            X, Q = base(dim)
            with pytest.MonkeyPatch.context() as mp:
                done[metric, dim, order] = whole_family(gpu, orc, mp, metric, order, X, Q, "unscaled")
        return done[metric, dim, order]

    return get


@pytest.mark.parametrize("metric,dim,order", CONFIGS)
def test_unscaled(unscaled, metric, dim, order):
    """The base rows as they are: what the families below are compared with.  The gap between the k-th and the (k + 16)-th
    distance of Gaussian rows is several bound widths (test_exact_search.py), so nearly every query is certified."""
    for k, (_, st, _) in unscaled(metric, dim, order).items():
        assert st["n_fallback_queries"] <= 0.05 * NQ, (k, st)


@pytest.mark.parametrize("e", [-30, 30])
@pytest.mark.parametrize("metric,dim,order", CONFIGS)
def test_scaled(gpu, orc, monkeypatch, unscaled, metric, dim, order, e):
    """Rows and queries times 2^e.  The oracle's distances scale by 2^(2e) exactly (cosine: not at all), so the ids are the unscaled
    run's; every factor of the bound is homogeneous in scale and the underflow allowance U is far below half an ulp of any term
    here, so the default path certifies exactly the queries it certifies unscaled."""
    ref = unscaled(metric, dim, order)
    X, Q = base(dim)
    Xs, Qs = np.ldexp(X, e).astype(np.float32), np.ldexp(Q, e).astype(np.float32)
    got = whole_family(gpu, orc, monkeypatch, metric, order, Xs, Qs, "scaled 2^%d" % e)
    for k in KS:
        (wi0, wd0, _), st0, _ = ref[k]
        (wi, wd, _), st, _ = got[k]
        assert np.array_equal(wi, wi0), (e, k)
        assert same_bits(wd, wd0 if metric == "cosine" else np.ldexp(wd0, 2 * e).astype(np.float32)), (e, k)
        assert st["n_fallback_queries"] == st0["n_fallback_queries"], (e, k, st0, st)


# ───────────────────────── 2. mixed scales, 3. offset ─────────────────────────

@pytest.mark.parametrize("metric,dim,order", CONFIGS)
def test_mixed_scales(gpu, orc, monkeypatch, metric, dim, order):
    """Row r times 2^e_r, e_r in -40..40: every row has a bound width of its own, the inner product's answers are the large rows,
    cosine has near-ties across 80 binades"""
    X, Q = base(dim)
    e = np.random.default_rng(3).integers(-40, 41, N)
    X = np.ldexp(X, e[:, None]).astype(np.float32)
    whole_family(gpu, orc, monkeypatch, metric, order, X, Q, "mixed")


@pytest.mark.parametrize("metric,dim,order", CONFIGS)
def test_offset(gpu, orc, monkeypatch, metric, dim, order):
    """Rows and queries + 100: |q|² + |x|² is thousands of times |q - x|², the L2 bound is thousands of neighbour spacings wide.
    No certificate rate is asked for: the point is mass fall-back, the gathered k_exact_valu launch with nearly every query marked."""
    X, Q = base(dim)
    out = whole_family(gpu, orc, monkeypatch, metric, order, X + np.float32(100), Q + np.float32(100), "offset")
    if metric != "inner_product":  # (its bound's width is relative to |q||x|, and so are its answers' gaps)
        for k in KS:
            assert out[k][1]["n_fallback_queries"] > 0, (k, out[k][1])


# ───────────────────────── 4. tiny and zero ─────────────────────────

@pytest.mark.parametrize("T", [5, 55])  # below and above every K' in use (26, 48; 10, 32 without slack)
@pytest.mark.parametrize("metric,dim,order", CONFIGS)
def test_tiny_and_zero(gpu, orc, monkeypatch, metric, dim, order, T):
    """T rows times 2^-60 (√n_b < 2^-40: i_x = +inf, lb = -inf, never rejected), T rows times 2^-140 (subnormal elements, every
    product underflows), T all-zero rows; a zero query, a 2^-60 query and a 2^-140 query."""
    X, Q = base(dim)
    rows = np.random.default_rng(4).choice(N, 3 * T, replace=False)
    X[rows[:T]] = np.ldexp(X[rows[:T]], -60)
    X[rows[T:2 * T]] = np.ldexp(X[rows[T:2 * T]], -140)
    X[rows[2 * T:]] = 0.0
    Q[3] = 0.0
    Q[4] = np.ldexp(Q[4], -60)
    Q[5] = np.ldexp(Q[5], -140)
    assert np.abs(X[rows[T:2 * T]]).max() < 2.0 ** -126 and np.abs(X[rows[T:2 * T]]).max() > 0  # subnormal, not flushed here
    dead = (7, 600, 1099)
    live = np.setdiff1d(np.arange(N), dead)
    D = all_distances(orc, metric, order, X, Q)
    # what the regime means, on the oracle's own output: hundreds-way ties that resolve by slot
    small = np.setdiff1d(rows, dead)
    if metric == "cosine":
        assert (D[3] == 1.0).all() and (D[5] == 1.0).all()            # na = 0: den < 1e-30
        assert (D[4][rows[T:]] == 1.0).all() and (D[:, rows[2 * T:]] == 1.0).all()
    elif metric == "inner_product":
        assert (bits(D[3]) == NEG_ZERO).all()
    out = whole_family(gpu, orc, monkeypatch, metric, order, X, Q, "tiny T=%d" % T, dead, D)
    for k in KS:
        wi, wd, _ = out[k][0]
        if metric != "l2":
            assert np.array_equal(wi[3], IDS[live[:k]]), k  # the zero query: every live row ties, the first k slots win
        if metric == "inner_product":
            assert (bits(wd[3]) == NEG_ZERO).all(), k
        if metric == "l2" and dim == 768 and len(small) >= k:
            assert np.isin(wi[6], IDS[small]).all(), k  # a unit query's nearest rows are the rows at the origin: |q|² against 2|q|²


# ───────────────────────── 5. huge and finite, 6. huge and overflowing ─────────────────────────

@pytest.mark.parametrize("metric,dim,order", CONFIGS)
def test_huge_finite(gpu, orc, monkeypatch, metric, dim, order):
    """Every 20th row and one query times 3e17: squared norms near 7e37 at dim 768, nothing overflows"""
    X, Q = base(dim)
    X[::20] *= np.float32(3e17)
    Q[2] *= np.float32(3e17)
    D = all_distances(orc, metric, order, X, Q)
    assert np.isfinite(D).all()
    whole_family(gpu, orc, monkeypatch, metric, order, X, Q, "huge-finite", D=D)


@pytest.mark.parametrize("metric,dim,order", [c for c in CONFIGS if c[0] != "inner_product"])
def test_huge_overflow(gpu, orc, monkeypatch, metric, dim, order):
    """Every 20th row times 1e19: its squares overflow.  L2 distances to those rows are +inf; cosine to them is finite (1.0), over a
    stored norm of +inf.  (The inner product is left out: with unit queries it adds nothing over the family above, and once the
    query is huge too its partial sums reach inf - inf.)"""
    X, Q = base(dim)
    X[::20] *= np.float32(1e19)
    D = all_distances(orc, metric, order, X, Q)
    if metric == "l2":
        assert (np.isinf(D).sum(axis=1) == 55).all() and np.isinf(D[:, ::20]).all()
    else:
        assert np.isfinite(D).all()
    whole_family(gpu, orc, monkeypatch, metric, order, X, Q, "huge-overflow", D=D)


# ───────────────────────── 7. rows at +inf belong in the answer ─────────────────────────

def _inf_rows_case(row_scale=1e19):
    n, dim = 100, 33
    X, Q = gauss(n, dim, 1), gauss(6, dim, 2)
    X[20:] *= np.float32(row_scale)
    ids = np.arange(100, 100 + n, dtype=np.int64)
    dead = (4, 11, 30, 77)  # two finite rows, two rows at +inf
    live = np.setdiff1d(np.arange(n), dead)
    return X, Q, ids, dead, live


def test_l2_rows_at_infinity_are_returned_before_the_filler(gpu, orc, monkeypatch):
    """100 rows, 80 of them at L2 distance +inf from every query: the answer holds the finite rows, then rows at +inf in slot order
    with their ids, and only past counts = min(k, live) the filler -1 / +inf"""
    X, Q, ids, dead, live = _inf_rows_case()
    D = all_distances(orc, "l2", 0, X, Q)
    assert np.isfinite(D[:, :20]).all() and np.isinf(D[:, 20:]).all()
    g = make_index(gpu, "l2", 0, X, ids, ids[list(dead)])
    out = three_paths(g, orc, monkeypatch, "l2", 0, X, ids, live, Q, D, "inf rows", ks=(10, 32, 128))
    g.close()
    fin, far = live[live < 20], live[live >= 20]
    assert len(fin) == 18 and len(far) == 78
    for k in (10, 32, 128):
        c = min(k, 96)
        for gi, gd, gc in out[k][2]:  # each path's own answer (three_paths has compared it with the oracle's already)
            assert (gc == c).all(), k
            for q in range(len(Q)):
                head = min(k, 18)
                assert set(gi[q, :head]) <= set(ids[fin]) and np.isfinite(gd[q, :head]).all(), (k, q)
                assert head < 18 or set(gi[q, :18]) == set(ids[fin]), (k, q)
                assert np.array_equal(gi[q, 18:c], ids[far[:max(c - 18, 0)]]), (k, q)  # +inf ties: slot order, real ids
                assert np.isinf(gd[q, 18:c]).all(), (k, q)
                assert (gi[q, c:] == -1).all() and np.isinf(gd[q, c:]).all(), (k, q)  # the filler, only past the count


@pytest.mark.parametrize("scale", [4e18, 1e19])
def test_l2_every_distance_at_infinity(gpu, orc, monkeypatch, scale):
    """The queries huge as well: every L2 distance is +inf (no NaN: differences are finite, their squares are not) and N_q + N_x
    overflows in the bound.  At 1e19 most dot products overflow too (s = inf - inf); at 4e18 they stay finite and s = +inf for all
    80 huge rows: no bound, lb = 0.  (A bound of +inf would never enter a list that is still filling; the list then looks short of
    K' and thus complete, and counts come out below min(k, live).)  The answer is the first min(k, live) live slots, at +inf."""
    X, Q, ids, dead, live = _inf_rows_case(scale)
    Q = Q * np.float32(scale)
    D = all_distances(orc, "l2", 0, X, Q)
    assert np.isinf(D).all()
    g = make_index(gpu, "l2", 0, X, ids, ids[list(dead)])
    out = three_paths(g, orc, monkeypatch, "l2", 0, X, ids, live, Q, D, "all inf", ks=(10, 32, 128))
    g.close()
    for k in (10, 32, 128):
        c = min(k, 96)
        for gi, gd, gc in out[k][2]:
            assert (gc == c).all() and (gi[:, :c] == ids[live[:c]]).all() and (gi[:, c:] == -1).all() and np.isinf(gd).all(), k


@pytest.mark.parametrize("dim", [33, 768])
def test_l2_squared_norms_between_half_and_all_of_flt_max(gpu, orc, monkeypatch, dim):
    """Queries of norm 1.35e19 (|q|² = 1.8e38, above FLT_MAX / 2) and, for each, three rows of the same norm at cosines 0.88, 0.90
    and 0.92 to it, among 300 rows of scale 1e17.  For such a pair a_q + a_x overflows while 2A = 2c|q|² stays finite: s = +inf,
    yet d = 2(1 - c)|q|² = 2.9e37..4.4e37 is finite and a fifth of the distance to any medium row (|q|² = 1.8e38, spread by a few
    per cent): the three rows are the query's nearest.  Any bound but "none" for a non-finite s puts them behind K' medium rows
    whose bounds are a thousand times narrower than their spread, and the certificate passes without them.  Medium queries see
    the same huge rows through finite sums."""
    n, nh = 300, 8
    X = gauss(n, dim, 81) * np.float32(1e17)
    Q = gauss(2 * nh, dim, 82) * np.float32(1e17)
    rng = np.random.default_rng(83)
    slots = np.sort(rng.choice(n, 3 * nh, replace=False)).reshape(nh, 3)
    for i in range(nh):
        u = rng.standard_normal(dim)
        u /= np.linalg.norm(u)
        Q[i] = (1.35e19 * u).astype(np.float32)
        for j, c in enumerate((0.88, 0.90, 0.92)):
            v = rng.standard_normal(dim)
            v -= (v @ u) * u
            v /= np.linalg.norm(v)
            X[slots[i, j]] = (1.35e19 * (c * u + np.sqrt(1 - c * c) * v)).astype(np.float32)
    nsq = np.concatenate([(Q[:nh].astype(np.float64) ** 2).sum(axis=1), (X[slots.ravel()].astype(np.float64) ** 2).sum(axis=1)])
    fmax = float(np.finfo(np.float32).max)
    assert (nsq > fmax / 2).all() and (nsq < fmax).all()
    ids = np.arange(100, 100 + n, dtype=np.int64)
    dead = [int(s_) for s_ in np.setdiff1d(np.arange(n), slots.ravel())[[5, 100, 250]]]  # medium rows
    live = np.setdiff1d(np.arange(n), dead)
    D = all_distances(orc, "l2", 0, X, Q)
    for i in range(nh):  # the regime, on the oracle's own output
        assert np.isfinite(D[i][slots[i]]).all() and set(np.argsort(D[i], kind="stable")[:3]) == set(slots[i]), i
        assert D[i][slots[i]].max() < 0.5 * np.delete(D[i], slots[i]).min(), i
    g = make_index(gpu, "l2", 0, X, ids, ids[dead])
    out = three_paths(g, orc, monkeypatch, "l2", 0, X, ids, live, Q, D, "half to all of FLT_MAX")
    g.close()
    for k in KS:
        for gi, _, _ in out[k][2]:
            for i in range(nh):
                assert set(gi[i, :3]) == set(ids[slots[i]]), (k, i)


# ───────────────────────── list and tile geometry ─────────────────────────

GEOM_N = (1, 25, 26, 27, 63, 64, 65, 127, 128, 129, 1024, 1025, 2049)
# 26 = K' at k 10: n == K' takes the certificate, n < K' is final without one; 64: the same at the clamp; 127..129: a tile's edge;
# 1024 / 1025: max_chunks = ceil(n / 1024) goes from 1 to 2; 2049: 3 chunks


def _kprime(k, slack):
    return min(k + (16 if slack is None else int(slack)), 64)


@pytest.mark.parametrize("n", GEOM_N)
@pytest.mark.parametrize("metric", METRICS)
def test_list_and_tile_geometry(gpu, orc, monkeypatch, metric, n):
    dim = 16
    X, QQ = gauss(n, dim, 61), gauss(129, dim, 62)
    ids = np.arange(1, n + 1, dtype=np.int64)
    dead = [n // 2] if n > 1 else []
    live = np.setdiff1d(np.arange(n), dead)
    D = all_distances(orc, metric, 0, X, QQ)
    g = make_index(gpu, metric, 0, X, ids, ids[dead])
    for nq in (1, 128, 129):
        Q = QQ[:nq]
        for k in (1, 10, 32):
            want = reference(orc, metric, 0, X, ids, live, Q, k, D[:nq])
            for slack in (None, "32", "100"):
                if slack is not None:
                    monkeypatch.setenv("MN_EXACT_SLACK", slack)
                got, st = exact(g, Q, k)
                monkeypatch.delenv("MN_EXACT_SLACK", raising=False)
                key = (nq, k, slack, st)
                check(got, want, key)
                assert st["n_mfma_queries"] == nq, key
                assert st["n_rescored_rows"] == nq * min(_kprime(k, slack), len(live)), key
    g.close()


def test_device_buffers_with_allow_list_and_deletions(gpu, orc):
    dim, metric, k, n, nq = 16, "l2", 10, 1025, 129
    X, Q = gauss(n, dim, 71), gauss(nq, dim, 72)
    ids = np.arange(1, n + 1, dtype=np.int64)
    dead = [0, 511, 1024]
    g = make_index(gpu, metric, 0, X, ids, ids[dead])
    pick = np.sort(np.random.default_rng(73).choice(n, n // 3, replace=False))
    allow = np.concatenate([ids[pick], ids[dead], [10 ** 12]]).astype(np.int64)  # + the deleted rows and one id never held
    ok = np.setdiff1d(pick, dead)
    dq, di, dd, dc = g.dev_malloc(Q.nbytes), g.dev_malloc(nq * k * 8), g.dev_malloc(nq * k * 4), g.dev_malloc(nq * 4)
    g.dev_upload(dq, Q)
    g.search_exact_batch_dev(dq, nq, k, di, dd, dc, allow)
    gi, gd, gc = np.empty((nq, k), np.int64), np.empty((nq, k), np.float32), np.empty(nq, np.int32)
    g.dev_download(gi, di)
    g.dev_download(gd, dd)
    g.dev_download(gc, dc)
    st = g.last_exact()
    assert st["n_bound_violations"] == 0 and st["n_queries"] == nq and st["n_mfma_queries"] == nq, st
    check((gi, gd, gc), reference(orc, metric, 0, X, ids, ok, Q, k), "dev")
    for p in (dq, di, dd, dc):
        g.dev_free(p)
    g.close()
