"""Entity resolution on the device (csrc/mn_er.hip, ext/mn_er_sql.c): Jaro-Winkler against the bits recorded from the compiled
reference and against the model, candidate pairs and the scoring cascade against the model, mn_hnsw_er_edges against its own
stages run one by one, and muninn_extract_er against the reference's JSON, byte for byte.  Every array is compared by bits."""
import gzip
import json
import os
import sqlite3
import subprocess

import numpy as np
import pytest

import er_model as em
from util import gauss

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXT_DIR = os.path.join(ROOT, "sqlite-muninn_amd", "ext")


@pytest.fixture(scope="module")
def golden():
    with gzip.open(os.path.join(ROOT, "tests", "golden", "er.json.gz"), "rb") as f:
        return json.loads(f.read())


def f64_bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


def model_bits(pairs):
    return np.array([em.bits(em.jaro_winkler(a, b)) for a, b in pairs], np.int64)


# ───────────────────────── Jaro-Winkler ─────────────────────────

def test_jw_equals_the_reference_bits(gpu, golden):
    """lengths 0, 1, 2, 3 (window 0), 4, 5, 63, 64, 65, 127-129, 255-257 in every combination, 4096; alphabets of 2-4 letters and
    bytes 1-255; identical names, empty against non-empty, no common byte, repeated bytes, adjacent swaps, prefixes 0-5; every
    pair in both argument orders — one call, short and long pairs side by side"""
    a = [bytes.fromhex(x[0]) for x in golden["jw"]]
    b = [bytes.fromhex(x[1]) for x in golden["jw"]]
    want = np.array([x[2] for x in golden["jw"]], np.int64)
    got = f64_bits(gpu.er.jaro_winkler(a, b))
    bad = np.nonzero(got != want)[0]
    assert len(bad) == 0, [(len(a[i]), len(b[i]), int(got[i]), int(want[i])) for i in bad[:5]]


@pytest.fixture(scope="module")
def mixed_pairs():
    """a shuffled mix: mostly lane-sized names, one in six longer than 64 bytes, a few of thousands of bytes"""
    rng = np.random.default_rng(5)
    al = [b"ab", b"abc", b"abcd", bytes(range(1, 256))]
    out = []
    for i in range(330):
        a_ = al[int(rng.integers(0, 4))]
        la = int(rng.integers(0, 65)) if i % 6 else int(rng.integers(65, 400))
        lb = int(rng.integers(0, 65)) if i % 5 else int(rng.integers(1, 300))
        s = em.rand_name(rng, la, a_)
        t = em.swap_adjacent(s, range(0, la, 4))[:lb] if i % 3 == 0 else em.rand_name(rng, lb, a_)
        out.append((s, t))
    out.append((em.rand_name(rng, 3000, b"abc"), em.rand_name(rng, 2500, b"abc")))
    out.append((em.rand_name(rng, 4096, b"ab"), em.rand_name(rng, 4095, b"ab")))
    order = rng.permutation(len(out))
    out = [out[i] for i in order]
    return out, model_bits(out)


def test_jw_shuffled_mix_equals_the_model(gpu, mixed_pairs):
    pairs, want = mixed_pairs
    got = f64_bits(gpu.er.jaro_winkler([p[0] for p in pairs], [p[1] for p in pairs]))
    bad = np.nonzero(got != want)[0]
    assert len(bad) == 0, [(len(pairs[i][0]), len(pairs[i][1])) for i in bad[:5]]
    rev = f64_bits(gpu.er.jaro_winkler([p[1] for p in pairs], [p[0] for p in pairs]))
    assert np.array_equal(rev, model_bits([(b, a) for a, b in pairs]))


@pytest.mark.parametrize("n_pairs", [0, 1, 63, 64, 65])
def test_jw_pair_counts_around_one_wavefront(gpu, mixed_pairs, n_pairs):
    pairs, want = mixed_pairs
    got = gpu.er.jaro_winkler([p[0] for p in pairs[:n_pairs]], [p[1] for p in pairs[:n_pairs]])
    assert got.shape == (n_pairs,) and np.array_equal(f64_bits(got), want[:n_pairs])


def test_jw_pairs_index_one_arena(gpu):
    """the C-ABI's own shape: pairs are indices into one table of names, a name may stand in many pairs and on either side"""
    raw = [b"", b"a", b"ab", b"ba", b"abcabcabc" * 9, b"abcabcabc" * 9 + b"x", b"MARTHA", b"MARHTA"]
    arena, off = gpu.er.pack_names(raw)
    a, b = np.meshgrid(np.arange(len(raw), dtype=np.int32), np.arange(len(raw), dtype=np.int32))
    a, b = a.reshape(-1).copy(), b.reshape(-1).copy()
    got = f64_bits(gpu.er.jaro_winkler_packed(arena, off, a, b))
    assert np.array_equal(got, model_bits([(raw[i], raw[j]) for i, j in zip(a, b)]))


# ───────────────────────── candidate pairs ─────────────────────────

def same_candidates(gpu, ent, ids, ds, cnt, thr):
    r1, r2, d = gpu.er.candidates(ent, ids, ds, cnt, thr)
    want = em.candidates(ent, ids, ds, cnt, thr)
    assert list(zip(r1.tolist(), r2.tolist())) == [(a, b) for a, b, _ in want]
    assert np.array_equal(f64_bits(d), f64_bits([w[2] for w in want]))
    return want


def test_candidates_by_hand(gpu):
    """j holds i but not the reverse, both, neither; the two directions one ulp apart (the smaller wins, whichever side has it);
    a distance equal to the threshold (kept) and the next float up (dropped); ids that are no entity; the entity's own id first
    and mid-list; counts 0, negative and below kk; rowids neither contiguous nor sorted"""
    thr32 = np.float32(0.25)
    up = np.nextafter(thr32, np.float32(1))
    lo = np.nextafter(np.float32(0.125), np.float32(0))
    ent = np.array([70, 5, 900, 33, 12, 1 << 40, -4], np.int64)
    X = 777  # no entity
    ids = np.array([[70, 5, 900, X],       # 0: own id first; 0-1 both ways; 0-2 only here
                    [900, 5, 70, 33],      # 1: own id mid-list; 1-2 both ways; 1-3 only here
                    [5, X, 33, 12],        # 2: 2-3 at the threshold, 2-4 one float above it
                    [1 << 40, -4, X, X],   # 3: count 2
                    [33, 70, 5, 900],      # 4: count 0: nothing of this list counts
                    [33, -4, 70, X],       # 5: 5-3 both ways; 5-6 only here; count 2 hides 70
                    [X, X, X, X]], np.int64)  # 6: count -1
    ds = np.array([[0, 0.125, 0.2, 0.01], [0.1, 0, lo, 0.22], [0.1 + 1e-8, 0.0, thr32, up], [0.2, 0.21, 0, 0], [0, 0, 0, 0],
                   [0.19, 0.05, 0.01, 0], [0, 0, 0, 0]], np.float32)
    cnt = np.array([4, 4, 4, 2, 0, 2, -1], np.int32)
    want = same_candidates(gpu, ent, ids, ds, cnt, float(thr32))
    pairs = {(a, b): d for a, b, d in want}
    assert pairs[(0, 1)] == float(lo) and pairs[(2, 3)] == float(thr32) and (2, 4) not in pairs and (0, 5) not in pairs
    assert pairs[(3, 5)] == float(np.float32(0.19)) and (5, 6) in pairs and (3, 6) in pairs and (0, 4) not in pairs
    assert [(a, b) for a, b, _ in want][:3] == [(0, 1), (0, 2), (1, 2)]


def test_candidates_refuses_an_entity_id_named_twice(gpu):
    ent = np.array([7, 3, 9, 3], np.int64)
    ids = np.array([[3], [7], [7], [9]], np.int64)
    with pytest.raises(gpu.MuninnHipError, match="ent_ids names an id twice"):
        gpu.er.candidates(ent, ids, np.zeros((4, 1), np.float32), np.ones(4, np.int32), 0.5)
    assert len(gpu.er.candidates(ent[:3], ids[:3], np.zeros((3, 1), np.float32), np.ones(3, np.int32), 0.5)[0]) == 2


@pytest.mark.parametrize("kk", [1, 11, 128])
@pytest.mark.parametrize("n", [0, 1, 2, 300])
def test_candidates_random_lists(gpu, n, kk):
    rng = np.random.default_rng(1000 * n + kk)
    ent = rng.permutation(np.arange(1, 4 * n + 2, dtype=np.int64) * 7)[:n]  # unsorted, gaps
    strangers = -np.arange(1, max(10, 130 - n) + 1, dtype=np.int64)
    pool = np.concatenate([ent, strangers])  # an entity's own id comes up among the draws, first, mid-list or last
    ids = np.full((n, kk), -1, np.int64)
    for i in range(n):
        ids[i] = rng.choice(pool, kk, replace=False)
    grid = np.float32(0.3) + np.arange(-3, 4, dtype=np.float32) * np.float32(2.0 ** -25)  # the threshold's float neighbours
    ds = np.where(rng.random((n, kk)) < 0.3, rng.choice(grid, (n, kk)), rng.random((n, kk), dtype=np.float32) * np.float32(0.5))
    ds = ds.astype(np.float32)
    cnt = rng.integers(-1, kk + 1, n).astype(np.int32)
    want = same_candidates(gpu, ent, ids, ds, cnt, float(np.float32(0.3)))
    if n == 300 and kk > 1:
        assert len(want) > 500


# ───────────────────────── scoring cascade ─────────────────────────

@pytest.fixture(scope="module")
def score_case():
    rng = np.random.default_rng(12)
    stems = [b"Jonathan Smith", b"Acme Corporation", b"Initech LLC", b"x" * 70 + b"Long Name Inc", b"Q", b""]
    names = []
    for i in range(120):
        s = stems[int(rng.integers(0, len(stems)))]
        how = int(rng.integers(0, 4))
        if how == 1:
            s = s.upper()
        elif how == 2:
            s = em.swap_adjacent(s, [int(rng.integers(0, max(1, len(s))))])
        elif how == 3:
            s = s + bytes([int(rng.integers(97, 123))])
        names.append(s)
    sources = [[b"", b"a", b"b"][int(rng.integers(0, 3))] for _ in names]
    r1 = rng.integers(0, 119, 700).astype(np.int32)
    r2 = (r1 + 1 + rng.integers(0, 119 - r1)).astype(np.int32)
    dist = rng.random(700) * 0.4
    dist[::9] = np.float32(dist[::9]).astype(np.float64)
    return names, sources, list(zip(r1.tolist(), r2.tolist(), dist.tolist()))


def same_edges(got, want):
    assert got["r1"].tolist() == [w[0] for w in want] and got["r2"].tolist() == [w[1] for w in want]
    assert np.array_equal(f64_bits(got["weight"]), f64_bits([w[2] for w in want]))


@pytest.mark.parametrize("jw_weight", [0.0, 0.5, 1.0])
@pytest.mark.parametrize("guard", [None, "same_source", "diff_type"])
def test_score_equals_the_model(gpu, score_case, guard, jw_weight):
    names, sources, cands = score_case
    hit = {}
    want = em.cascade(cands, names, sources, guard, jw_weight, 0.8, hit)
    assert hit["exact"] and hit["lower"] and hit["jw"] and hit["kept"] and hit["dropped"]
    assert guard is None or hit["guard_" + guard]
    got = gpu.er.score([c[0] for c in cands], [c[1] for c in cands], [c[2] for c in cands], names, sources, guard, jw_weight, 0.8)
    same_edges(got, want)  # the same candidates, in candidate order, the same f64


def test_score_at_the_threshold_and_without_survivors(gpu, score_case):
    names, sources, cands = score_case
    every = em.cascade(cands, names, sources, None, 0.5, -1.0)
    assert len(every) == len(cands)
    jw_scores = sorted(s for _, _, s in every if s not in (1.0, 0.9))
    at = jw_scores[len(jw_scores) // 2]  # a score some candidate has exactly: >= keeps it
    want = em.cascade(cands, names, sources, None, 0.5, at)
    assert any(s == at for _, _, s in want) and len(want) < len(cands)
    r1, r2, d = [c[0] for c in cands], [c[1] for c in cands], [c[2] for c in cands]
    same_edges(gpu.er.score(r1, r2, d, names, sources, None, 0.5, at), want)
    above = float(np.nextafter(at, 2.0))
    same_edges(gpu.er.score(r1, r2, d, names, sources, None, 0.5, above), em.cascade(cands, names, sources, None, 0.5, above))
    assert len(gpu.er.score(r1, r2, d, names, sources, None, 0.5, 2.0)) == 0
    assert len(gpu.er.score([], [], [], names, sources, None, 0.5, 0.0)) == 0
    same_edges(gpu.er.score(r1, r2, d, names, None, "same_source", 0.5, 0.8), em.cascade(cands, names, None, "same_source", 0.5, 0.8))


# ───────────────────────── mn_hnsw_er_edges ─────────────────────────

@pytest.fixture(scope="module")
def er_index(gpu):
    """420 rows in 60 tight groups of 7 plus noise; names vary inside a group.  Entities: the rows in another order, ten ids
    the index does not hold, five rows deleted from the index."""
    rng = np.random.default_rng(3)
    dim, n = 32, 420
    centres = gauss(60, dim, 41)
    X = (centres[np.arange(n) % 60] + 0.25 * gauss(n, dim, 42)).astype(np.float32)
    ids = (np.arange(n, dtype=np.int64) + 1) * 11
    g = gpu.HnswIndex(dim, "cosine", 8, 60)
    assert g.build(ids, X) == 0
    gone = ids[[3, 77, 200, 201, 419]]
    for i in gone:
        assert g.delete(int(i)) == 0
    ent = np.concatenate([rng.permutation(ids), -np.arange(1, 11, dtype=np.int64)])
    ent = ent[rng.permutation(len(ent))]
    stems = [b"Group %d Holdings" % (i % 60) for i in range(60)]
    names, sources = [], []
    for e in ent:
        s = stems[int(abs(e) // 11 - 1) % 60] if e > 0 else b"Nobody"
        how = int(rng.integers(0, 5))
        s = [s, s, s.upper(), em.swap_adjacent(s, [6]), s + b" " + b"y" * 60][how]
        names.append(s)
        sources.append([b"", b"a", b"b"][int(rng.integers(0, 3))])
    yield g, ent, names, sources, set(int(i) for i in gone)
    g.close()


K, THR, W = 6, 0.12, 0.4


@pytest.mark.parametrize("guard", [None, "same_source"])
def test_er_edges_graph_blocking_equals_its_stages(gpu, er_index, guard):
    """the reference's blocking: every entity's stored vector searched at k + 1 with ef = 2 (k + 1); an id the index does not
    hold and a deleted row have no vector and no list"""
    g, ent, names, sources, gone = er_index
    n, kk = len(ent), K + 1
    ids = np.full((n, kk), -1, np.int64)
    ds = np.zeros((n, kk), np.float32)
    cnt = np.zeros(n, np.int32)
    have = [i for i, e in enumerate(ent) if g.get_vector(int(e)) is not None]
    assert len(have) == n - 10 - len(gone)
    Q = np.stack([g.get_vector(int(ent[i])) for i in have])
    ids[have], ds[have], cnt[have] = g.search_batch(Q, kk, 2 * kk)
    r1, r2, d = gpu.er.candidates(ent, ids, ds, cnt, THR)
    mt = 1.0 - THR + 0.02
    want = gpu.er.score(r1, r2, d, names, sources, guard, W, mt)
    got, st = gpu.er.resolve(g, ent, names, sources, K, THR, W, 0.02, guard, "graph", return_stats=True)
    assert len(want) > 100 and got.tobytes() == want.tobytes()
    assert st["n_candidates"] == len(r1) and st["n_edges"] == len(want)
    assert st["n_jw_short"] > 0 and st["n_jw_long"] > 0
    same_edges(got, em.cascade(em.candidates(ent, ids, ds, cnt, THR), names, sources, guard, W, mt))
    live = {int(e) for e in ent[have]}
    assert all(int(ent[e["r1"]]) in live and int(ent[e["r2"]]) in live for e in got)


def test_er_edges_exact_blocking_equals_the_model_on_knn_graph(gpu, er_index):
    g, ent, names, sources, gone = er_index
    n = len(ent)
    cut = np.float32(THR)  # the largest float not above the threshold: what the library cuts the k-NN graph at
    if float(cut) > THR:
        cut = np.nextafter(cut, np.float32(-1))
    live_ids, nbr, nd, nc = g.knn_graph(K, cut)
    row = {int(v): i for i, v in enumerate(live_ids)}
    ids = np.full((n, K), -1, np.int64)
    ds = np.zeros((n, K), np.float32)
    cnt = np.zeros(n, np.int32)
    for i, e in enumerate(ent):
        if int(e) in row:
            ids[i], ds[i], cnt[i] = nbr[row[int(e)]], nd[row[int(e)]], nc[row[int(e)]]
    mt = 1.0 - THR
    want = em.cascade(em.candidates(ent, ids, ds, cnt, THR), names, sources, "diff_type", W, mt)
    got = gpu.er.resolve(g, ent, names, sources, K, THR, W, 0.0, "diff_type", "exact")
    assert len(want) > 100
    same_edges(got, want)
    r1, r2, d = gpu.er.candidates(ent, ids, ds, cnt, THR)
    assert got.tobytes() == gpu.er.score(r1, r2, d, names, sources, "diff_type", W, mt).tobytes()
    assert not any(int(ent[e["r1"]]) in gone or int(ent[e["r2"]]) in gone or ent[e["r1"]] < 0 or ent[e["r2"]] < 0 for e in got)


def test_er_edges_small_and_empty(gpu):
    g = gpu.HnswIndex(8, "cosine", 8, 40)
    ent = np.array([4, 9], np.int64)
    for blocking in ("graph", "exact"):  # an empty index: nobody has a vector
        assert len(gpu.er.resolve(g, ent, [b"a", b"a"], None, 3, 0.5, 0.5, blocking=blocking)) == 0
    v = np.ones(8, np.float32)
    assert g.insert(4, v) == 0 and g.insert(9, v) == 0
    for blocking in ("graph", "exact"):
        e = gpu.er.resolve(g, ent, [b"a", b"a"], None, 3, 0.5, 0.5, blocking=blocking)
        assert e.tolist() == [(0, 1, 1.0)]
        assert len(gpu.er.resolve(g, ent[:0], [], None, 3, 0.5, 0.5, blocking=blocking)) == 0
    with pytest.raises(gpu.MuninnHipError, match=r"k must be 1\.\.127 \(got 128\)"):
        gpu.er.resolve(g, ent, [b"a", b"a"], None, 128, 0.5, 0.5)
    g.close()


# ───────────────────────── muninn_extract_er ─────────────────────────

def er_conn(mn, golden, state):
    mn.build()
    subprocess.run(["make", "-s", "-C", EXT_DIR], check=True)
    c = sqlite3.connect(":memory:")
    c.enable_load_extension(True)
    c.load_extension(os.path.join(EXT_DIR, "muninn"))
    c.execute(f"CREATE VIRTUAL TABLE vec USING hnsw_index(dimensions={golden['dim']}, metric='cosine')")
    c.execute("CREATE TABLE entities(entity_id TEXT, name TEXT, source TEXT)")
    for rowid, eid, name, source, vec in golden["entities"]:
        c.execute("INSERT INTO entities(rowid, entity_id, name, source) VALUES (?, ?, ?, ?)", (rowid, eid, name, source))
        if vec is not None:
            c.execute("INSERT INTO vec(rowid, vector) VALUES (?, ?)", (rowid, bytes.fromhex(vec)))
    for rowid in golden["states"][state]:
        c.execute("DELETE FROM vec WHERE rowid = ?", (rowid,))
    c.commit()
    return c


def call(c, args):
    return c.execute("SELECT muninn_extract_er('vec', 'name', " + ", ".join("?" for _ in args) + ")", args).fetchone()[0]


@pytest.mark.parametrize("state", ["main", "after_delete"])
def test_sql_equals_the_reference_json(mn, gpu, golden, monkeypatch, state):
    """the vtab in exact insert mode holds the reference's graph, so the reference's searches, and from them every byte of its
    answer: each case of the recorded grid (guards, weights, k, thresholds, the bridge cut, a row without a vector, a deleted
    row, an id that needs escaping)"""
    monkeypatch.setenv("MUNINN_HNSW_MODE", "exact")
    monkeypatch.delenv("MUNINN_ER_BLOCKING", raising=False)
    c = er_conn(mn, golden, state)
    bad = {}
    for name, case in golden["grid"][state].items():
        got = call(c, case["args"])
        if got != case["json"]:
            bad[name] = (got, case["json"])
    assert not bad, bad
    assert c.execute("SELECT count(*) FROM sqlite_temp_master WHERE name = '_er_edges'").fetchone()[0] == 0
    assert c.execute("SELECT json_valid(muninn_extract_er('vec', 'name', 4, 0.3, 0.5, 0.0))").fetchone()[0] == 1
    # subtype 'J' (src/llama_er.c:573): a JSON function embeds the result as an object, not as a string
    assert c.execute("SELECT json_type(json_object('a', muninn_extract_er('vec', 'name', 4, 0.3, 0.5, 0.0)), '$.a')").fetchone()[0] == \
        "object"
    c.close()


def test_sql_exact_blocking(mn, gpu, golden, monkeypatch):
    monkeypatch.setenv("MUNINN_HNSW_MODE", "exact")
    monkeypatch.setenv("MUNINN_ER_BLOCKING", "exact")
    c = er_conn(mn, golden, "main")
    keys = [e[1] for e in golden["entities"]]
    for name in ("base", "same_source", "eb_cut", "k1"):
        got = json.loads(call(c, golden["grid"]["main"][name]["args"]))
        assert list(got) == ["clusters"] and list(got["clusters"]) == keys
        assert sorted(set(got["clusters"].values())) == list(range(len(set(got["clusters"].values()))))
    monkeypatch.setenv("MUNINN_ER_BLOCKING", "nearest")
    with pytest.raises(sqlite3.OperationalError, match="MUNINN_ER_BLOCKING must be 'graph' or 'exact'"):
        call(c, golden["grid"]["main"]["base"]["args"])
    c.close()
