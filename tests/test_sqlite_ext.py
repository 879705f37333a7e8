"""SQLite loadable extension (sqlite-muninn_amd/ext/muninn.so): the reference's SQL contracts
(pytests/test_hnsw_vtab.py) restated.  CPU tests cover loading, registration, argument errors and the
hand-written ABI header; -m gpu tests run the SQL surface end to end on the device, and compare the
shadow tables with those written by the compiled reference (same inputs)."""
import os
import random
import sqlite3
import struct
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXT_DIR = os.path.join(ROOT, "sqlite-muninn_amd", "ext")
EXT = os.path.join(EXT_DIR, "muninn")


def vec(values):
    return struct.pack(f"<{len(values)}f", *values)


@pytest.fixture(scope="session")
def ext_built(mn):
    mn.build()
    subprocess.run(["make", "-s", "-C", EXT_DIR], check=True)
    return EXT


@pytest.fixture
def conn(ext_built):
    c = sqlite3.connect(":memory:")
    c.enable_load_extension(True)
    c.load_extension(ext_built)
    yield c
    c.close()


# ───────────────────────── CPU ─────────────────────────

def test_entry_symbol_and_modules_register(conn):
    mods = {r[0] for r in conn.execute("SELECT name FROM pragma_module_list")}
    assert "hnsw_index" in mods and "hnsw0" in mods


@pytest.mark.parametrize("sql,pat", [
    ("CREATE VIRTUAL TABLE bad USING hnsw_index(metric='l2')", "dimensions.*required"),
    ("CREATE VIRTUAL TABLE bad USING hnsw_index(dimensions=4, metric='hamming')", "unknown metric"),
    ("CREATE VIRTUAL TABLE bad USING hnsw_index(dimensions=0)", "dimensions must be > 0"),
    ("CREATE VIRTUAL TABLE bad USING hnsw_index(dimensions=4, foobar=1)", "unknown parameter"),
    ("CREATE VIRTUAL TABLE bad USING hnsw_index(dimensions=4, m=1)", "m must be >= 2"),
    ("CREATE VIRTUAL TABLE bad USING hnsw_index(dimensions=4, ef_construction=0)", "ef_construction must be >= 1"),
])
def test_create_argument_errors(conn, sql, pat):
    with pytest.raises(Exception, match=pat):  # pytests/test_hnsw_vtab.py:49-63
        conn.execute(sql)


def test_abi_header_matches_real_sqlite_header(tmp_path):
    """mn_sqlite_abi.h is hand-written; every slot number and struct layout it relies on is held against the values measured
    on a genuine sqlite3ext.h (the reference vendors one), recorded in tests/golden/sqlite_abi.json by oracle/gen_golden.py."""
    import json

    from oracle import sqlite_abi

    want = json.load(open(os.path.join(ROOT, "tests", "golden", "sqlite_abi.json")))
    slots = sqlite_abi.declared_slots()
    assert len(slots) >= 40
    assert slots == want["slots"]
    _, layout = sqlite_abi.measure(sqlite_abi.ABI_H, str(tmp_path))
    assert dict(zip(sqlite_abi.LAYOUT, layout)) == want["layout"]


# ───────────────────────── GPU: pytests/test_hnsw_vtab.py restated ─────────────────────────

gpu_mark = pytest.mark.gpu


@gpu_mark
def test_create_makes_shadow_tables_and_drop_removes_them(conn, gpu):
    conn.execute("CREATE VIRTUAL TABLE test_vec USING hnsw_index(dimensions=4, metric='l2')")
    tables = {r[0] for r in conn.execute("SELECT name FROM sqlite_master WHERE type='table'")}
    assert {"test_vec_config", "test_vec_nodes", "test_vec_edges"} <= tables
    conn.execute("INSERT INTO test_vec (rowid, vector) VALUES (1, ?)", (vec([1, 2, 3, 4]),))
    conn.execute("DROP TABLE test_vec")
    tables = {r[0] for r in conn.execute("SELECT name FROM sqlite_master WHERE type='table'")}
    assert not ({"test_vec_config", "test_vec_nodes", "test_vec_edges"} & tables)


@gpu_mark
def test_insert_search_delete_point_lookup(conn, gpu):
    conn.execute("CREATE VIRTUAL TABLE v USING hnsw_index(dimensions=2, metric='l2')")
    for i, p in enumerate([[0, 0], [10, 0], [0, 10]], start=1):
        conn.execute("INSERT INTO v (rowid, vector) VALUES (?, ?)", (i, vec(p)))
    assert conn.execute("SELECT id, level FROM v_nodes WHERE id=1").fetchone()[0] == 1
    with pytest.raises(Exception, match="expected 2-dim"):
        conn.execute("INSERT INTO v (rowid, vector) VALUES (9, ?)", (vec([1.0]),))
    with pytest.raises(Exception, match="duplicate rowid"):
        conn.execute("INSERT INTO v (rowid, vector) VALUES (1, ?)", (vec([1, 1]),))
    with pytest.raises(Exception, match="must be a BLOB"):
        conn.execute("INSERT INTO v (rowid, vector) VALUES (7, 'text')")
    res = conn.execute("SELECT rowid, distance FROM v WHERE vector MATCH ? AND k = 2", (vec([0.1, 0.1]),)).fetchall()
    assert len(res) == 2 and res[0][0] == 1 and res[0][1] < 1.0
    with pytest.raises(Exception, match="expected 2-dim"):
        conn.execute("SELECT rowid FROM v WHERE vector MATCH ? AND k = 2", (vec([0.1]),)).fetchall()
    row = conn.execute("SELECT vector, distance FROM v WHERE rowid = 2").fetchone()
    assert struct.unpack("<2f", row[0]) == (10.0, 0.0) and row[1] == 0.0
    assert conn.execute("SELECT rowid FROM v").fetchall() == []  # full scan returns nothing (:614-617)
    conn.execute("DELETE FROM v WHERE rowid = 2")
    ids = {r[0] for r in conn.execute("SELECT rowid FROM v WHERE vector MATCH ? AND k = 3", (vec([10.0, 0.0]),))}
    assert ids == {1, 3}
    conn.execute("DELETE FROM v WHERE rowid = 2")  # point lookup finds nothing → no row reaches xUpdate
    with pytest.raises(Exception, match="UPDATE not supported"):
        conn.execute("UPDATE v SET vector = ? WHERE rowid = 1", (vec([1, 1]),))
    # auto rowid (:722-727)
    conn.execute("INSERT INTO v (vector) VALUES (?)", (vec([5, 5]),))
    assert conn.execute("SELECT COUNT(*) FROM v_nodes").fetchone()[0] == 4


@gpu_mark
def test_knn_recall_100_vectors(conn, gpu):
    dim, k = 8, 5
    random.seed(42)
    conn.execute(f"CREATE VIRTUAL TABLE v USING hnsw_index(dimensions={dim}, metric='l2', m=16, ef_construction=200)")
    vectors = {}
    for i in range(100):
        p = [random.gauss(0, 1) for _ in range(dim)]
        vectors[i] = p
        conn.execute("INSERT INTO v (rowid, vector) VALUES (?, ?)", (i, vec(p)))
    q = [random.gauss(0, 1) for _ in range(dim)]
    res = conn.execute("SELECT rowid, distance FROM v WHERE vector MATCH ? AND k = ? AND ef_search = 64", (vec(q), k)).fetchall()
    assert len(res) == k
    bf = sorted(vectors, key=lambda i: sum((a - b) ** 2 for a, b in zip(q, vectors[i])))[:k]
    assert len(set(bf) & {r[0] for r in res}) / k >= 0.8
    assert [r[1] for r in res] == sorted(r[1] for r in res)


@gpu_mark
def test_cosine_and_empty(conn, gpu):
    conn.execute("CREATE VIRTUAL TABLE e USING hnsw_index(dimensions=2, metric='l2')")
    assert conn.execute("SELECT rowid FROM e WHERE vector MATCH ? AND k = 5", (vec([0, 0]),)).fetchall() == []
    conn.execute("CREATE VIRTUAL TABLE c USING hnsw0(dimensions=2, metric='cosine')")
    for i, p in enumerate([[1, 0], [0, 1], [-1, 0]], start=1):
        conn.execute("INSERT INTO c (rowid, vector) VALUES (?, ?)", (i, vec(p)))
    res = conn.execute("SELECT rowid FROM c WHERE vector MATCH ? AND k = 3", (vec([0.95, 0.05]),)).fetchall()
    assert res[0][0] == 1


@gpu_mark
def test_persistence_across_reopen(ext_built, gpu, tmp_path):
    db = str(tmp_path / "t.db")
    c1 = sqlite3.connect(db)
    c1.enable_load_extension(True)
    c1.load_extension(ext_built)
    c1.execute("CREATE VIRTUAL TABLE v USING hnsw_index(dimensions=3, metric='l2', m=4)")
    for i in range(10):
        c1.execute("INSERT INTO v (rowid, vector) VALUES (?, ?)", (i, vec([float(i), float(i * 2), float(i * 3)])))
    c1.commit()
    c1.close()
    c2 = sqlite3.connect(db)
    c2.enable_load_extension(True)
    c2.load_extension(ext_built)
    res = c2.execute("SELECT rowid, distance FROM v WHERE vector MATCH ? AND k = 3", (vec([0, 0, 0]),)).fetchall()
    assert len(res) == 3 and res[0][0] == 0
    c2.close()


@gpu_mark
@pytest.mark.parametrize("mode", ["exact", "deferred"])
def test_shadow_tables_identical_to_reference(ext_built, gpu, tmp_path, monkeypatch, mode):
    """tests/golden/vtab_shadow.npz holds what the REFERENCE's extension wrote for a seeded input
    (oracle/gen_golden.py: vtab_shadow).  The same inserts through ours must leave identical _config,
    _nodes and _edges rows, including the per-edge REAL distance; and the database file the reference
    wrote (tests/golden/ref_written.db) must open here and answer the recorded queries identically."""
    import shutil

    monkeypatch.setenv("MUNINN_HNSW_MODE", mode)
    G = os.path.join(ROOT, "tests", "golden")
    z = np.load(os.path.join(G, "vtab_shadow.npz"))
    X = np.random.default_rng(5).standard_normal((300, 12), dtype=np.float32)
    c = sqlite3.connect(str(tmp_path / "ours.db"))
    c.enable_load_extension(True)
    c.load_extension(ext_built)
    c.execute("CREATE VIRTUAL TABLE v USING hnsw_index(dimensions=12, metric='cosine', m=6, ef_construction=40)")
    with c:
        for i in range(len(X)):
            c.execute("INSERT INTO v (rowid, vector) VALUES (?, ?)", (i + 1, X[i].tobytes()))
    cfg = [f"{k}={v}" for k, v in c.execute("SELECT key, value FROM v_config ORDER BY key")]
    assert cfg == z["config"].tolist()
    nodes = np.array(c.execute("SELECT id, level, deleted FROM v_nodes ORDER BY id").fetchall(), np.int64)
    assert np.array_equal(nodes, z["nodes"])
    vecs = c.execute("SELECT vector FROM v_nodes ORDER BY id").fetchall()
    assert all(v[0] == X[i].tobytes() for i, v in enumerate(vecs))
    edges = c.execute("SELECT source_id, target_id, level, distance FROM v_edges ORDER BY 1,3,2").fetchall()
    assert np.array_equal(np.array([e[:3] for e in edges], np.int64), z["edges_int"])
    assert np.array_equal(np.array([e[3] for e in edges], np.float64), z["edges_dist"])
    for q, ri, rd in zip(z["queries"], z["res_ids"], z["res_dist"]):
        got = c.execute("SELECT rowid, distance FROM v WHERE vector MATCH ? AND k = 5 AND ef_search = 40", (q.tobytes(),)).fetchall()
        assert [g[0] for g in got] == ri.tolist() and [g[1] for g in got] == rd.tolist()
    c.close()
    # cross-open: a file written by the reference
    shutil.copy(os.path.join(G, "ref_written.db"), tmp_path / "ref.db")
    c = sqlite3.connect(str(tmp_path / "ref.db"))
    c.enable_load_extension(True)
    c.load_extension(ext_built)
    for q, ri, rd in zip(z["queries"], z["reopen_ids"], z["reopen_dist"]):
        got = c.execute("SELECT rowid, distance FROM v WHERE vector MATCH ? AND k = 5 AND ef_search = 40", (q.tobytes(),)).fetchall()
        # after reload neighbour lists are in primary-key order (src/hnsw_vtab.c:322-338); the expected
        # answers were recorded from the reference after ITS reopen of the same file
        assert [g[0] for g in got] == ri.tolist() and [g[1] for g in got] == rd.tolist()
    c.close()


@gpu_mark
def test_config1_at_its_own_parameters_equals_the_reference_extension(ext_built, gpu, monkeypatch):
    """BASELINE config 1 exactly as SURVEY §8(d) defines it — 10 000 x 128 default_rng(42), cosine, M = 16,
    efConstruction = 200, one INSERT per row in one transaction, 100 queries x ef {20, 64, 128, 256} — through ext/muninn.so
    in exact mode, against what the REFERENCE's extension produced for the same statements (tests/golden/vtab_cfg1.npz,
    oracle/gen_golden.py vtab_cfg1): _config, every node level, every _edges row (hash over ids, levels and REAL distance
    bits), every returned rowid and distance."""
    import hashlib

    monkeypatch.setenv("MUNINN_HNSW_MODE", "exact")
    z = np.load(os.path.join(ROOT, "tests", "golden", "vtab_cfg1.npz"))
    rng = np.random.default_rng(42)
    X = rng.standard_normal((10_000, 128), dtype=np.float32)
    Q = rng.standard_normal((100, 128), dtype=np.float32)
    c = sqlite3.connect(":memory:")
    c.enable_load_extension(True)
    c.load_extension(ext_built)
    c.execute("CREATE VIRTUAL TABLE v USING hnsw_index(dimensions=128, metric='cosine', m=16, ef_construction=200)")
    with c:
        for i in range(len(X)):
            c.execute("INSERT INTO v (rowid, vector) VALUES (?, ?)", (i + 1, X[i].tobytes()))
    assert [f"{k}={v}" for k, v in c.execute("SELECT key, value FROM v_config ORDER BY key")] == z["config"].tolist()
    levels = np.array([r[0] for r in c.execute("SELECT level FROM v_nodes ORDER BY id")], np.int8)
    assert np.array_equal(levels, z["levels"])
    h = hashlib.sha256()
    n_edges, head = 0, []
    for s_, t_, l_, d_ in c.execute("SELECT source_id, target_id, level, distance FROM v_edges ORDER BY 1,3,2"):
        h.update(np.array([s_, t_, l_], np.int64).tobytes() + np.array([d_], np.float64).tobytes())
        if n_edges < 400:
            head.append((s_, t_, l_, d_))
        n_edges += 1
    assert np.array_equal(np.array([e[:3] for e in head], np.int64), z["edges_head_int"])
    assert np.array_equal(np.array([e[3] for e in head], np.float64), z["edges_head_dist"])
    assert n_edges == int(z["n_edges"][0]) and h.hexdigest() == str(z["edges_sha256"][0])
    for ef in (20, 64, 128, 256):
        for qi, q in enumerate(Q):
            got = c.execute("SELECT rowid, distance FROM v WHERE vector MATCH ? AND k = 10 AND ef_search = ?", (q.tobytes(), ef)).fetchall()
            assert [g[0] for g in got] == z[f"ids_ef{ef}"][qi].tolist(), (ef, qi)
            assert [g[1] for g in got] == z[f"dist_ef{ef}"][qi].tolist(), (ef, qi)
    c.close()


# ───────────────────────── node2vec_train / graph_leiden through SQL ─────────────────────────

def test_graph_functions_registered_and_validate_args(conn):
    mods = {r[0] for r in conn.execute("SELECT name FROM pragma_module_list")}
    assert "graph_leiden" in mods
    assert conn.execute("SELECT 1 FROM pragma_function_list WHERE name='node2vec_train'").fetchone()
    conn.execute("CREATE TABLE e (src TEXT, dst TEXT)")
    for args, pat in [(("e;drop", "src", "dst", "o", 8, 1.0, 1.0, 1, 5, 2, 2, 0.025, 1), "invalid edge_table"),
                      (("e", "src", "dst", "o", 0, 1.0, 1.0, 1, 5, 2, 2, 0.025, 1), "dimensions must be 1-1024"),
                      (("e", "src", "dst", "o", 8, 0.0, 1.0, 1, 5, 2, 2, 0.025, 1), "p and q must be > 0"),
                      (("e", "src", "dst", "o", 8, 1.0, 1.0, 0, 5, 2, 2, 0.025, 1), "num_walks and walk_length"),
                      (("e", "src", "dst", "o", 8, 1.0, 1.0, 1, 5, 0, 2, 0.025, 1), "window and neg_samples"),
                      (("e", "src", "dst", "o", 8, 1.0, 1.0, 1, 5, 2, 2, 0.0, 1), "learning_rate and epochs")]:
        with pytest.raises(Exception, match=pat):  # src/node2vec.c:427-464
            conn.execute("SELECT node2vec_train(?,?,?,?,?,?,?,?,?,?,?,?,?)", args).fetchone()
    # empty graph → 0 without touching the device (pytests/test_node2vec.py:178-190)
    assert conn.execute("SELECT node2vec_train('e','src','dst','o',8,1.0,1.0,5,10,3,3,0.025,1)").fetchone()[0] == 0
    # missing required constraint → no rows / planner refusal, bad identifier → error
    with pytest.raises(Exception):
        conn.execute("SELECT * FROM graph_leiden WHERE edge_table='e;x' AND src_col='src' AND dst_col='dst'").fetchall()
    assert conn.execute("SELECT * FROM graph_leiden WHERE edge_table='e' AND src_col='src' AND dst_col='dst'").fetchall() == []


@gpu_mark
def test_node2vec_train_sql_matches_reference_bytes(conn, gpu):
    from oracle.graph_cases import n2v_cases

    z = np.load(os.path.join(ROOT, "tests", "golden", "node2vec.npz"))
    for name in ("cliques16", "karate_pq", "cliques_walk4100", "cliques_d1024"):
        edges, (dim, p, q, nw, wl, win, neg, lr, ep) = n2v_cases()[name]
        conn.execute(f"CREATE TABLE e_{name} (src TEXT, dst TEXT)")
        conn.executemany(f"INSERT INTO e_{name} VALUES (?, ?)", [(str(a), str(b)) for a, b in edges])
        conn.execute(f"CREATE VIRTUAL TABLE emb_{name} USING hnsw_index(dimensions={dim}, metric='cosine', m=8, ef_construction=50)")
        n = conn.execute(f"SELECT node2vec_train('e_{name}', 'src', 'dst', 'emb_{name}', ?, ?, ?, ?, ?, ?, ?, ?, ?)",
                         (dim, p, q, nw, wl, win, neg, lr, ep)).fetchone()[0]
        want = z[name].view(np.float32)
        assert n == want.shape[0]
        rows = conn.execute(f"SELECT id, vector FROM emb_{name}_nodes ORDER BY id").fetchall()
        got = np.array([np.frombuffer(r[1], np.float32) for r in rows], np.float32)
        assert np.array_equal(got.view(np.int32), want.view(np.int32)), name
        for rowid in range(1, n + 1):  # retrievable through the vtab (pytests/test_node2vec.py:164-176)
            assert len(conn.execute(f"SELECT vector FROM emb_{name} WHERE rowid = ?", (rowid,)).fetchone()[0]) == dim * 4


@gpu_mark
def test_graph_leiden_sql_matches_reference(conn, gpu):
    from oracle.graph_cases import leiden_cases

    z = np.load(os.path.join(ROOT, "tests", "golden", "leiden.npz"))
    # barbell: exactly {A,B,C},{D,E,F} (pytests/test_graph_community.py:129-150)
    conn.execute("CREATE TABLE bb (src TEXT, dst TEXT)")
    conn.executemany("INSERT INTO bb VALUES (?,?)", [("A", "B"), ("B", "C"), ("C", "A"), ("D", "E"), ("E", "F"), ("F", "D"), ("C", "D")])
    rows = conn.execute("SELECT node, community_id, modularity FROM graph_leiden WHERE edge_table='bb' AND src_col='src' AND dst_col='dst'").fetchall()
    comm = {r[0]: r[1] for r in rows}
    assert len(rows) == 6 and comm["A"] == comm["B"] == comm["C"] != comm["D"] and comm["D"] == comm["E"] == comm["F"]
    assert all(r[2] == rows[0][2] for r in rows) and rows[0][2] > 0
    assert sorted(set(comm.values())) == [0, 1]
    for name in ("karate", "er2000w", "er500w_r2"):
        s, d, w, res = leiden_cases()[name]
        conn.execute(f"CREATE TABLE g_{name} (src TEXT, dst TEXT, w REAL)")
        conn.executemany(f"INSERT INTO g_{name} VALUES (?,?,?)",
                         [(str(int(a)), str(int(b)), float(w[i]) if w is not None else 1.0) for i, (a, b) in enumerate(zip(s, d))])
        wc = "AND weight_col='w'" if w is not None else ""
        rows = conn.execute(f"SELECT node, community_id, modularity FROM graph_leiden WHERE edge_table='g_{name}' AND src_col='src' "
                            f"AND dst_col='dst' {wc} AND resolution = ?", (res,)).fetchall()
        got = np.array([r[1] for r in rows], np.int32)  # rows come out in first-seen node order
        assert np.array_equal(got, z[f"{name}_community"]), name
        assert np.array([rows[0][2]], np.float64).view(np.int64)[0] == z[f"{name}_q"][0]


@gpu_mark
def test_hnsw_search_batch_tvf_equals_per_query_results(conn, gpu):
    """Additive batch surface: one launch for many queries must return exactly what the per-query MATCH returns."""
    rng = np.random.default_rng(3)
    X = rng.standard_normal((400, 16), dtype=np.float32)
    Q = rng.standard_normal((25, 16), dtype=np.float32)
    conn.execute("CREATE VIRTUAL TABLE bv USING hnsw_index(dimensions=16, metric='l2', m=8, ef_construction=60)")
    with conn:
        for i in range(len(X)):
            conn.execute("INSERT INTO bv (rowid, vector) VALUES (?, ?)", (i + 1, X[i].tobytes()))
    rows = conn.execute("SELECT query_idx, id, distance FROM hnsw_search_batch WHERE tbl='bv' AND queries=? AND k=5 AND ef_search=40",
                        (Q.tobytes(),)).fetchall()
    assert len(rows) == 25 * 5
    for qi in range(25):
        one = conn.execute("SELECT rowid, distance FROM bv WHERE vector MATCH ? AND k = 5 AND ef_search = 40", (Q[qi].tobytes(),)).fetchall()
        got = [(r[1], r[2]) for r in rows if r[0] == qi]
        assert got == one
    with pytest.raises(Exception, match="multiple of"):
        conn.execute("SELECT * FROM hnsw_search_batch WHERE tbl='bv' AND queries=? AND k=5", (b"123",)).fetchall()
    with pytest.raises(Exception, match="no hnsw_index table"):
        conn.execute("SELECT * FROM hnsw_search_batch WHERE tbl='nope' AND queries=? AND k=5", (Q.tobytes(),)).fetchall()


@gpu_mark
def test_hnsw_search_batch_default_ef_search_and_k_zero(conn, gpu):
    """Without ef_search the rows are those of ef_search = 2 * k; k = 0 is refused in the words of the queries check."""
    from util import gauss, small_hnsw_table
    small_hnsw_table(conn, "sv")
    Q, k = gauss(5, 8, 102).tobytes(), 3
    sql = "SELECT rowid, query_idx, id, distance FROM hnsw_search_batch WHERE tbl='sv' AND queries=? AND k=?"
    rows = conn.execute(sql, (Q, k)).fetchall()
    assert len(rows) == 5 * k and rows == conn.execute(sql + " AND ef_search=?", (Q, k, 2 * k)).fetchall()
    with pytest.raises(sqlite3.OperationalError) as ei:
        conn.execute(sql, (Q, 0)).fetchall()
    assert str(ei.value) == "hnsw_search_batch: queries must be a multiple of 32 bytes (8-dim f32), got 160"


@gpu_mark
def test_graph_leiden_sql_fast_mode_matches_oracle_schedule(conn, gpu, monkeypatch):
    """MUNINN_GRAPH_MODE=fast → MN_LEIDEN_BATCHED's default schedule (whole-graph synchronous sweeps, pick-less every 3rd);
    must equal the CPU restatement of it (oracle batch -3)."""
    from oracle import orc_graph as og
    from oracle.graph_cases import leiden_cases

    s, d, w, res = leiden_cases()["er2000"]
    conn.execute("CREATE TABLE gf (src TEXT, dst TEXT)")
    conn.executemany("INSERT INTO gf VALUES (?,?)", [(str(int(a)), str(int(b))) for a, b in zip(s, d)])
    monkeypatch.setenv("MUNINN_GRAPH_MODE", "fast")
    rows = conn.execute("SELECT node, community_id, modularity FROM graph_leiden WHERE edge_table='gf' AND src_col='src' AND dst_col='dst'").fetchall()
    csr = og.Csr(s, d, None, "both")
    oc, oq, _ = og.leiden(csr, res, -3)
    assert np.array_equal(np.array([r[1] for r in rows], np.int32), oc)
    assert rows[0][2] == oq
    monkeypatch.setenv("MUNINN_GRAPH_MODE", "exact")
    rows2 = conn.execute("SELECT community_id FROM graph_leiden WHERE edge_table='gf' AND src_col='src' AND dst_col='dst'").fetchall()
    z = np.load(os.path.join(ROOT, "tests", "golden", "leiden.npz"))
    assert np.array_equal(np.array([r[0] for r in rows2], np.int32), z["er2000_community"])


# ───────────────────────── deferred inserts / bulk persistence ─────────────────────────

@gpu_mark
@pytest.mark.parametrize("mode", ["exact", "deferred"])
def test_mixed_transaction_ops_match_reference(ext_built, gpu, monkeypatch, mode):
    """Inserts (explicit and automatic rowids), deletes and a search interleaved inside transactions, then
    autocommit inserts: the rowids handed out, the answers and the final _config/_nodes/_edges rows are those of
    the reference's extension for the same SQL (tests/golden/vtab_mixed.npz, oracle/gen_golden.py:vtab_mixed) —
    in exact mode (persist per row) and in deferred mode (rows queued by xUpdate, persisted once per flush)."""
    from oracle.gen_golden import vtab_mixed_ops

    monkeypatch.setenv("MUNINN_HNSW_MODE", mode)
    conn = sqlite3.connect(":memory:")
    conn.enable_load_extension(True)
    conn.load_extension(ext_built)
    z = np.load(os.path.join(ROOT, "tests", "golden", "vtab_mixed.npz"))
    got = vtab_mixed_ops(conn, z["X"], z["Q"])
    conn.close()
    assert got["log"].tolist() == z["log"].tolist()
    assert got["config"].tolist() == z["config"].tolist()
    assert np.array_equal(got["nodes"], z["nodes"])
    assert np.array_equal(got["edges_int"], z["edges_int"])
    assert np.array_equal(got["edges_dist"], z["edges_dist"])
    assert np.array_equal(got["res_ids"], z["res_ids"]) and np.array_equal(got["res_dist"], z["res_dist"])


@gpu_mark
def test_queued_rows_rollback_duplicates_and_visibility(conn, gpu, monkeypatch):
    monkeypatch.setenv("MUNINN_HNSW_MODE", "deferred")
    conn.execute("CREATE VIRTUAL TABLE q USING hnsw_index(dimensions=2, metric='l2', m=4)")
    conn.isolation_level = None  # explicit transactions
    conn.execute("BEGIN")
    conn.execute("INSERT INTO q (rowid, vector) VALUES (1, ?)", (vec([0, 0]),))
    conn.execute("INSERT INTO q (rowid, vector) VALUES (2, ?)", (vec([1, 0]),))
    with pytest.raises(Exception, match=r"insert failed \(duplicate rowid 2\?\)"):
        conn.execute("INSERT INTO q (rowid, vector) VALUES (2, ?)", (vec([5, 5]),))  # reported by the INSERT itself
    # queued rows are visible to reads of the same transaction
    assert [r[0] for r in conn.execute("SELECT rowid FROM q WHERE vector MATCH ? AND k = 2", (vec([0.9, 0]),))] == [2, 1]
    assert conn.execute("SELECT count(*) FROM q_nodes").fetchone()[0] == 2
    conn.execute("INSERT INTO q (rowid, vector) VALUES (3, ?)", (vec([0, 1]),))
    conn.execute("ROLLBACK")  # row 3 was only queued: it never reaches the index
    assert conn.execute("SELECT count(*) FROM q_nodes").fetchone()[0] == 0
    assert conn.execute("SELECT rowid FROM q WHERE rowid = 3").fetchall() == []
    conn.execute("BEGIN")
    conn.execute("INSERT INTO q (rowid, vector) VALUES (3, ?)", (vec([0, 1]),))
    conn.execute("COMMIT")
    assert conn.execute("SELECT rowid FROM q WHERE rowid = 3").fetchall() == [(3,)]
    assert conn.execute("SELECT count(*) FROM q_edges WHERE source_id = 3").fetchone()[0] >= 1


@gpu_mark
@pytest.mark.parametrize("mode", ["deferred", "fast"])
def test_rolled_back_savepoints_and_failed_statements_take_their_queued_rows_with_them(conn, gpu, monkeypatch, mode):
    """rows queued after a SAVEPOINT (or by the first rows of a multi-row INSERT that then fails) must not be inserted
    and persisted by the COMMIT that follows a ROLLBACK TO / the statement's rollback."""
    monkeypatch.setenv("MUNINN_HNSW_MODE", mode)
    conn.execute("CREATE VIRTUAL TABLE q USING hnsw_index(dimensions=2, metric='l2', m=4)")
    conn.isolation_level = None
    ins = "INSERT INTO q (rowid, vector) VALUES (?, ?)"
    conn.execute("BEGIN")
    conn.execute(ins, (1, vec([0, 0])))
    conn.execute("SAVEPOINT s")
    conn.execute(ins, (2, vec([1, 0])))
    conn.execute("ROLLBACK TO s")
    conn.execute(ins, (3, vec([0, 1])))
    conn.execute("SAVEPOINT a")
    conn.execute(ins, (20, vec([2, 2])))
    conn.execute("SAVEPOINT b")
    conn.execute(ins, (21, vec([3, 3])))
    conn.execute("RELEASE b")
    conn.execute("ROLLBACK TO a")  # takes 20 and (released into a) 21
    conn.execute(ins, (2, vec([9, 9])))  # rowid 2 is free again: the rolled-back row left the queue's id set too
    with pytest.raises(Exception, match=r"insert failed \(duplicate rowid 1\?\)"):  # third row fails: the statement's first two go
        conn.execute("INSERT INTO q (rowid, vector) VALUES (11, ?), (12, ?), (1, ?)", (vec([4, 4]), vec([5, 5]), vec([6, 6])))
    conn.execute("COMMIT")
    assert [r[0] for r in conn.execute("SELECT id FROM q_nodes ORDER BY id")] == [1, 2, 3]
    assert conn.execute("SELECT vector FROM q_nodes WHERE id = 2").fetchone()[0] == vec([9, 9])
    for gone in (11, 12, 20, 21):
        assert conn.execute("SELECT rowid FROM q WHERE rowid = ?", (gone,)).fetchall() == []
    assert sorted(r[0] for r in conn.execute("SELECT rowid FROM q WHERE vector MATCH ? AND k = 10", (vec([0, 0]),))) == [1, 2, 3]
    assert conn.execute("SELECT count(*) FROM q_edges WHERE source_id NOT IN (1, 2, 3) OR target_id NOT IN (1, 2, 3)").fetchone()[0] == 0


@gpu_mark
def test_fast_mode_bulk_load_and_reopen(ext_built, gpu, tmp_path, monkeypatch):
    """MUNINN_HNSW_MODE=fast: one transaction of 6000 rows → batch-synchronous device build, shadow tables written
    once; recall equals the exact-mode table's within 0.02 and the file reopens (in exact mode) with the same answers."""
    monkeypatch.setenv("MUNINN_HNSW_MODE", "fast")
    rng = np.random.default_rng(17)
    n, dim = 6000, 24
    base = rng.standard_normal((n, 6), dtype=np.float32) @ rng.standard_normal((6, dim), dtype=np.float32)
    X = (base + 0.05 * rng.standard_normal((n, dim), dtype=np.float32)).astype(np.float32)
    Q = X[rng.choice(n, 40, replace=False)] + 0.01
    db = str(tmp_path / "fast.db")
    c = sqlite3.connect(db)
    c.enable_load_extension(True)
    c.load_extension(ext_built)
    c.execute("CREATE VIRTUAL TABLE f USING hnsw_index(dimensions=24, metric='l2', m=8, ef_construction=80)")
    with c:
        c.executemany("INSERT INTO f (rowid, vector) VALUES (?, ?)", [(i + 1, X[i].tobytes()) for i in range(n)])
    assert c.execute("SELECT count(*) FROM f_nodes").fetchone()[0] == n
    truth = [set((np.argsort(((X - q) ** 2).sum(1))[:10] + 1).tolist()) for q in Q]
    ans = [c.execute("SELECT rowid, distance FROM f WHERE vector MATCH ? AND k = 10 AND ef_search = 80", (q.tobytes(),)).fetchall() for q in Q]
    recall = np.mean([len(truth[i] & {r[0] for r in ans[i]}) / 10 for i in range(len(Q))])
    assert recall > 0.9, recall
    ne = c.execute("SELECT count(*) FROM f_edges").fetchone()[0]
    assert n * 4 < ne <= n * 20  # <= 2M per node at level 0 plus the upper layers
    c.close()
    monkeypatch.setenv("MUNINN_HNSW_MODE", "exact")
    c = sqlite3.connect(db)
    c.enable_load_extension(True)
    c.load_extension(ext_built)
    again = [c.execute("SELECT rowid FROM f WHERE vector MATCH ? AND k = 10 AND ef_search = 80", (q.tobytes(),)).fetchall() for q in Q]
    recall2 = np.mean([len(truth[i] & {r[0] for r in again[i]}) / 10 for i in range(len(Q))])
    assert abs(recall2 - recall) < 0.03
    c.close()


# ───────────────────────── graph_adjacency's stored CSR as input ─────────────────────────

def _gunzip_golden(name, tmp_path):
    import gzip
    import shutil

    dst = str(tmp_path / name)
    with gzip.open(os.path.join(ROOT, "tests", "golden", name + ".gz"), "rb") as fi, open(dst, "wb") as fo:
        shutil.copyfileobj(fi, fo)
    return dst


@gpu_mark
@pytest.mark.parametrize("state", ["fresh", "stale"])
def test_graph_leiden_on_a_graph_adjacency_table_matches_reference(ext_built, gpu, tmp_path, monkeypatch, state):
    """tests/golden/adjacency_{fresh,stale}.db were written by the REFERENCE's graph_adjacency vtab (two CSR blocks;
    the stale one has 40 rows in its delta log).  graph_leiden pointed at that table must answer what the reference
    answers: from the stored CSR blocks when fresh (uploaded as stored, mn_graph_create_blocked), from the original
    edge table when stale (src/graph_adjacency.c:1532-1573).  oracle/gen_golden.py:adjacency_kats."""
    monkeypatch.setenv("MUNINN_GRAPH_MODE", "exact")
    z = np.load(os.path.join(ROOT, "tests", "golden", "adjacency.npz"))
    c = sqlite3.connect(_gunzip_golden(f"adjacency_{state}.db", tmp_path))
    c.enable_load_extension(True)
    c.load_extension(ext_built)
    rows = c.execute("SELECT node, community_id, modularity FROM graph_leiden WHERE edge_table='g' AND src_col='src' AND dst_col='dst'").fetchall()
    assert [r[0] for r in rows] == z[f"{state}_nodes"].tolist()
    assert np.array_equal(np.array([r[1] for r in rows], np.int32), z[f"{state}_comm"])
    assert np.float64(rows[0][2]).view(np.int64) == z[f"{state}_q"][0]
    c.close()


@gpu_mark
def test_graph_from_stored_blocks_equals_graph_from_edges(gpu, tmp_path):
    """The C-ABI entry itself: blocks read from the reference-written file → same partition as the golden."""
    z = np.load(os.path.join(ROOT, "tests", "golden", "adjacency.npz"))
    c = sqlite3.connect(_gunzip_golden("adjacency_fresh.db", tmp_path))
    n = c.execute("SELECT COUNT(*) FROM g_nodes").fetchone()[0]
    fwd = c.execute("SELECT offsets, targets, weights FROM g_csr_fwd ORDER BY block_id").fetchall()
    rev = c.execute("SELECT offsets, targets, weights FROM g_csr_rev ORDER BY block_id").fetchall()
    c.close()
    assert len(fwd) == int(z["n_blocks"][0]) >= 2
    g = gpu.Graph.from_blocks(n, fwd, rev)
    comm, q, _ = g.leiden(1.0, "both", gpu.LEIDEN_SEQUENTIAL)
    g.close()
    assert np.array_equal(comm, z["fresh_comm"]) and np.float64(q).view(np.int64) == z["fresh_q"][0]
    with pytest.raises(Exception, match="out of range|malformed"):
        bad = [(fwd[0][0], np.full(len(fwd[0][1]) // 4, n + 5, np.int32).tobytes(), fwd[0][2])] + list(fwd[1:])
        gpu.Graph.from_blocks(n, bad, rev)


@gpu_mark
@pytest.mark.parametrize("seed,mode", [(s, m) for s in range(12) for m in ("exact", "deferred")] +
                         [(s, "exact") for s in range(100, 106)])  # 100+: sessions with ROLLBACKs
def test_random_sql_sessions_match_reference_transcripts(ext_built, gpu, monkeypatch, seed, mode):
    """tests/golden/vtab_fuzz.json.gz: transcripts of seeded random sessions (inserts with explicit / automatic /
    duplicate / malformed rows, deletes, kNN and point queries, transactions — seeds 100+ also ROLLBACKs, after which the
    reference's in-memory index still holds the rolled-back nodes and re-persists them when later inserts link to them;
    the deferred mode drops queued rows on rollback instead, so those seeds run in exact mode only) under the REFERENCE's extension — every
    returned rowid, distance (f64 bits), error text, and the final shadow tables.  The same session here must produce
    the same transcript line for line (oracle/gen_golden.py: vtab_fuzz_run)."""
    import gzip
    import json

    from oracle.gen_golden import vtab_fuzz_run

    with gzip.open(os.path.join(ROOT, "tests", "golden", "vtab_fuzz.json.gz"), "rt") as f:
        want = json.load(f)[str(seed)]
    monkeypatch.setenv("MUNINN_HNSW_MODE", mode)
    c = sqlite3.connect(":memory:")
    c.enable_load_extension(True)
    c.load_extension(ext_built)
    got = vtab_fuzz_run(c, seed, rollbacks=seed >= 100)
    c.close()
    for i, (a, b) in enumerate(zip(got, want)):
        assert a == b, f"line {i}: ours {a[:300]!r} reference {b[:300]!r}"
    assert len(got) == len(want)


@gpu_mark
@pytest.mark.parametrize("seed", range(8))
def test_random_graph_sql_sessions_match_reference_transcripts(ext_built, gpu, monkeypatch, seed):
    """tests/golden/graph_fuzz.json.gz: seeded sessions on the graph SQL surface under the REFERENCE's extension —
    graph_leiden with random options on edge tables with text ids, NULLs, duplicates, weights and time windows;
    node2vec_train with valid and invalid arguments into an hnsw_index table.  Same transcript here, line for line
    (communities, modularity bits, embedding bytes, error texts).  oracle/gen_golden.py: graph_fuzz_run."""
    import gzip
    import json

    from oracle.gen_golden import graph_fuzz_run

    monkeypatch.setenv("MUNINN_GRAPH_MODE", "exact")
    with gzip.open(os.path.join(ROOT, "tests", "golden", "graph_fuzz.json.gz"), "rt") as f:
        want = json.load(f)[str(seed)]
    c = sqlite3.connect(":memory:")
    c.enable_load_extension(True)
    c.load_extension(ext_built)
    got = graph_fuzz_run(c, seed)
    c.close()
    for i, (a, b) in enumerate(zip(got, want)):
        assert a == b, f"line {i}: ours {a[:400]!r} reference {b[:400]!r}"
    assert len(got) == len(want)


def test_integrated_build_keeps_the_rest_of_the_reference_surface_loadable():
    """"the other graph_* surface must remain loadable".  `make -C oracle integrated` links the reference's
    UNMODIFIED sqlite3_muninn_init and non-hot translation units (compiled where they lie; build container only) with
    this repository's hot-path extension sources: every module of src/muninn.c:42-121 (llama.cpp ones excepted — the
    submodule is absent) is registered by the reference's own entry point, the non-hot ones run as they always did."""
    so = os.path.join(ROOT, "oracle", "_ref", "integrated", "muninn")
    if not os.path.isdir("/root/reference/src"):
        pytest.skip("reference sources absent (GPU box): the integrated build is build-container evidence only")
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "oracle"), "integrated"], check=True)
    c = sqlite3.connect(":memory:")
    c.enable_load_extension(True)
    c.load_extension(so)
    mods = {r[0] for r in c.execute("SELECT name FROM pragma_module_list")}
    want = {"hnsw_index", "graph_bfs", "graph_dfs", "graph_shortest_path", "graph_components", "graph_pagerank", "graph_degree",
            "graph_node_betweenness", "graph_edge_betweenness", "graph_closeness", "graph_leiden", "graph_adjacency", "graph_select"}
    assert want <= mods, want - mods
    assert c.execute("SELECT count(*) FROM pragma_function_list WHERE name='node2vec_train' AND narg=13").fetchone()[0] == 1
    c.execute("CREATE TABLE e(s TEXT, d TEXT)")
    c.executemany("INSERT INTO e VALUES (?, ?)", [("a", "b"), ("b", "c"), ("c", "d")])
    bfs = c.execute("SELECT node, depth FROM graph_bfs WHERE edge_table='e' AND src_col='s' AND dst_col='d' AND start_node='a' "
                    "AND max_depth=5 AND direction='forward'").fetchall()
    assert bfs == [("a", 0), ("b", 1), ("c", 2), ("d", 3)]  # the reference's own traversal code, no GPU involved
    c.execute("CREATE VIRTUAL TABLE g USING graph_adjacency(edge_table='e', src_col='s', dst_col='d')")
    assert c.execute("SELECT count(*) FROM g").fetchone()[0] == 4  # the reference's graph_adjacency vtab, unchanged
    c.close()


@gpu_mark
def test_node2vec_train_into_a_live_hnsw_index_stays_on_the_device_and_equals_the_insert_path(ext_built, gpu, monkeypatch):
    """node2vec_train(..., output_table) where output_table is a live hnsw_index in fast mode: the extension hands the
    embeddings to the index inside HBM (mn_vtab_hnsw_fill_from_n2v) instead of one INSERT per row.  The result — returned count,
    "{t}_nodes" (rowids, vectors, levels), "{t}_edges", "{t}_config", search answers — must equal the generic INSERT path in
    the same mode (MUNINN_N2V_DIRECT=0)."""
    from oracle.graph_cases import planted

    monkeypatch.setenv("MUNINN_HNSW_MODE", "fast")
    monkeypatch.setenv("MUNINN_GRAPH_MODE", "fast")
    s, d, _ = planted(1500, 5, 0.06, 0.002, 3)
    out = {}
    for direct in ("1", "0"):
        monkeypatch.setenv("MUNINN_N2V_DIRECT", direct)
        c = sqlite3.connect(":memory:")
        c.enable_load_extension(True)
        c.load_extension(ext_built)
        c.execute("CREATE TABLE e (src TEXT, dst TEXT)")
        c.executemany("INSERT INTO e VALUES (?,?)", [(f"n{a}", f"n{b}") for a, b in zip(s, d)])
        c.execute("CREATE VIRTUAL TABLE emb USING hnsw_index(dimensions=32, metric='cosine', m=8, ef_construction=60)")
        with c:
            got = c.execute("SELECT node2vec_train('e','src','dst','emb',32,1.0,1.0,4,20,4,3,0.025,1)").fetchone()[0]
        q = c.execute("SELECT vector FROM emb_nodes WHERE id = 7").fetchone()[0]
        out[direct] = {"n": got,
                       "nodes": c.execute("SELECT id, vector, level, deleted FROM emb_nodes ORDER BY id").fetchall(),
                       "edges": c.execute("SELECT source_id, target_id, level, distance FROM emb_edges ORDER BY 1,3,2").fetchall(),
                       "config": c.execute("SELECT key, value FROM emb_config ORDER BY key").fetchall(),
                       "knn": c.execute("SELECT rowid, distance FROM emb WHERE vector MATCH ? AND k = 5 AND ef_search = 40", (q,)).fetchall()}
        c.close()
    assert out["1"]["n"] == out["0"]["n"] == len(out["1"]["nodes"]) > 1000
    for k in ("nodes", "edges", "config", "knn"):
        assert out["1"][k] == out["0"][k], k


@pytest.mark.gpu
@pytest.mark.parametrize("seed", [33, 34])
def test_incremental_graph_adjacency_rebuild_runs_the_device_merge_and_equals_the_reference(gpu, seed):
    """SURVEY §8 f-2 through the boundary: in the integrated build (oracle/Makefile) the reference's UNMODIFIED graph_adjacency.c
    calls csr_apply_delta (src/graph_adjacency.c:864,910) and reaches ext/mn_csr_adapter.c — the reference's signature over
    mn_csr_apply_delta on the GPU.  A graph of two CSR blocks (5 000 nodes), then INSERTs (new nodes included), DELETEs and an
    incremental rebuild: the stored blocks, the node registry and the vtab's rows must equal, byte for byte, what the
    reference's own extension (its CPU merge) produces for the same statements.  Both libraries are built in the build
    container (`make -C oracle ref integrated`) and travel to the GPU box as built objects.  (The edge table carries a weight
    column: without one the reference's own delta triggers do not compile — "no such column: NEW.NULL" — so its incremental
    path is only reachable on weighted tables.)"""
    weighted = True
    ref_so = os.path.join(ROOT, "oracle", "_ref", "muninn")
    int_so = os.path.join(ROOT, "oracle", "_ref", "integrated", "muninn")
    if not (os.path.exists(ref_so + ".so") and os.path.exists(int_so + ".so")):
        pytest.skip("oracle/_ref (compiled reference + integrated build) not present")
    syms = subprocess.run(["nm", "-D", int_so + ".so"], capture_output=True, text=True).stdout
    assert " T csr_apply_delta" in syms and "mn_csr_apply_delta" in syms  # the strong definition is the adapter's

    rng = np.random.default_rng(seed)
    n, m = 5000, 14000
    s0, d0 = rng.integers(0, n, m), rng.integers(0, n, m)
    w0 = rng.integers(1, 13, m) * 0.25
    ins = [(f"n{int(a)}", f"n{int(b)}" if i % 5 else f"new{int(b) % 40}", float(x))
           for i, (a, b, x) in enumerate(zip(rng.integers(0, n, 300), rng.integers(0, n, 300), rng.integers(1, 9, 300) * 0.5))]
    dele = rng.permutation(m)[:250]

    def session(so):
        c = sqlite3.connect(":memory:")
        c.enable_load_extension(True)
        c.load_extension(so)
        if weighted:
            c.execute("CREATE TABLE edges (src TEXT, dst TEXT, weight REAL)")
            c.executemany("INSERT INTO edges VALUES (?,?,?)", [(f"n{a}", f"n{b}", float(x)) for a, b, x in zip(s0, d0, w0)])
            c.execute("CREATE VIRTUAL TABLE g USING graph_adjacency(edge_table='edges', src_col='src', dst_col='dst', weight_col='weight')")
        else:
            c.execute("CREATE TABLE edges (src TEXT, dst TEXT)")
            c.executemany("INSERT INTO edges VALUES (?,?)", [(f"n{a}", f"n{b}") for a, b in zip(s0, d0)])
            c.execute("CREATE VIRTUAL TABLE g USING graph_adjacency(edge_table='edges', src_col='src', dst_col='dst')")
        c.execute("INSERT INTO g(g) VALUES ('rebuild')")
        assert c.execute("SELECT COUNT(*) FROM g_csr_fwd").fetchone()[0] >= 2
        if weighted:  # (the reference's DELETE trigger names OLD.<weight_col>: without a weight column it cannot be created
            #  usefully — "no such column: OLD.NULL" — so deletes are exercised on the weighted table only)
            for i in dele:  # (a duplicated (src, dst) pair loses every copy: one DELETE statement, several delta rows)
                c.execute("DELETE FROM edges WHERE src = ? AND dst = ?", (f"n{s0[i]}", f"n{d0[i]}"))
        if weighted:
            c.executemany("INSERT INTO edges VALUES (?,?,?)", ins)
        else:
            c.executemany("INSERT INTO edges VALUES (?,?)", [r[:2] for r in ins])
        nd = c.execute("SELECT COUNT(*) FROM g_delta").fetchone()[0]
        assert nd >= (500 if weighted else 300)
        c.execute("INSERT INTO g(g) VALUES ('incremental_rebuild')")
        assert c.execute("SELECT COUNT(*) FROM g_delta").fetchone()[0] == 0
        out = {"rows": c.execute("SELECT * FROM g ORDER BY 1").fetchall(),
               "fwd": c.execute("SELECT * FROM g_csr_fwd ORDER BY 1").fetchall(),
               "rev": c.execute("SELECT * FROM g_csr_rev ORDER BY 1").fetchall(),
               "nodes": c.execute("SELECT * FROM g_nodes ORDER BY 1").fetchall(),
               "degree": c.execute("SELECT * FROM g_degree ORDER BY 1").fetchall()}
        c.close()
        return out

    want, got = session(ref_so), session(int_so)
    for k in ("nodes", "degree", "rows", "fwd", "rev"):
        assert len(got[k]) == len(want[k]) and got[k] == want[k], k


@pytest.mark.gpu
def test_session_with_lists_longer_than_m_max_equals_the_reference(ext_built, gpu, monkeypatch):
    """tests/golden/vtab_overgrown.npz: one SQL session recorded from the REFERENCE's extension in which 800 of 1 000 rows of
    an m = 2 index are deleted (its reconnection step grows neighbour lists past M_max), searched, extended by 60 rows
    (which prune the long lists they touch) and searched again.  Same statements through this extension: same answers
    (ids and distances) on both states and identical shadow tables."""
    from oracle import gen_golden as gg

    monkeypatch.setenv("MUNINN_HNSW_MODE", "exact")
    z = np.load(os.path.join(ROOT, "tests", "golden", "vtab_overgrown.npz"))
    c = sqlite3.connect(":memory:")
    c.enable_load_extension(True)
    c.load_extension(ext_built)
    res1, res2, nodes, edges, cfg = gg.vtab_overgrown_ops(c)
    c.close()
    for res, ki, kd in ((res1, "res1_ids", "res1_dist"), (res2, "res2_ids", "res2_dist")):
        for q, rr in enumerate(res):
            assert [r[0] for r in rr] == [int(x) for x in z[ki][q] if x >= 0], (ki, q)
            assert [r[1] for r in rr] == z[kd][q][:len(rr)].tolist(), (kd, q)
    assert [f"{k}={v}" for k, v in cfg] == z["config"].tolist()
    assert np.array_equal(np.array(nodes, np.int64), z["nodes"])
    assert np.array_equal(np.array([e[:3] for e in edges], np.int64), z["edges_int"])
    assert np.array_equal(np.array([e[3] for e in edges], np.float64), z["edges_dist"])


_DEVICE_ENV = r"""
import os, sqlite3, sys
c = sqlite3.connect(":memory:"); c.enable_load_extension(True)
c.load_extension(os.path.join(os.environ["MN_ROOT"], "sqlite-muninn_amd", "ext", "muninn"))
try:
    c.execute("CREATE VIRTUAL TABLE t USING hnsw_index(dimensions=4, metric='l2')")
    c.execute("INSERT INTO t(rowid, vector) VALUES (1, ?)", (b"\0" * 16,))
    print("CREATED", c.execute("SELECT count(*) FROM t_nodes").fetchone()[0])
except sqlite3.Error as e:
    print("SQLERR", e)
try:
    c.execute("CREATE TABLE e(src TEXT, dst TEXT)"); c.executemany("INSERT INTO e VALUES (?,?)", [("a", "b"), ("b", "c")])
    print("PR", len(c.execute("SELECT * FROM graph_pagerank WHERE edge_table='e' AND src_col='src' AND dst_col='dst'").fetchall()))
except sqlite3.Error as e:
    print("SQLERR2", e)
"""


@pytest.mark.gpu
def test_muninn_device_env_selects_the_ordinal_and_fails_loudly_on_a_bad_one(ext_conn):
    """MUNINN_DEVICE=<ordinal>: 0 works as the default does; an ordinal the box does not have is an SQL error from
    CREATE VIRTUAL TABLE and from the graph TVFs (no crash, no silent fallback to another device or to the CPU)."""
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    # (malformed values — not a plain ordinal — are errors too, never "device 0": "abc", "1x", "-1", "")
    for dev, ok in (("0", True), ("63", False), ("abc", False), ("0x", False), ("-1", False), ("", False)):
        env = dict(os.environ, MUNINN_DEVICE=dev, MN_ROOT=root)
        r = subprocess.run([sys.executable, "-c", _DEVICE_ENV], env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        if ok:
            assert "CREATED 1" in r.stdout and "PR 3" in r.stdout, r.stdout
        else:
            assert "SQLERR" in r.stdout and "SQLERR2" in r.stdout and "CREATED" not in r.stdout and "PR 3" not in r.stdout, r.stdout
            assert "MUNINN_DEVICE=" in r.stdout, r.stdout  # the message names the variable


def _delta_session(ext_built, path, delta):
    """a session that exercises everything the edge-by-edge persistence has to survive; returns the tables after each phase"""
    env = dict(os.environ, MUNINN_HNSW_MODE="exact", MUNINN_HNSW_DELTA="1" if delta else "0", MN_ROOT=ROOT, MN_DB=path)
    code = r"""
import os, sqlite3, numpy as np
def connect():
    c = sqlite3.connect(os.environ["MN_DB"], isolation_level=None); c.enable_load_extension(True)
    c.load_extension(os.path.join(os.environ["MN_ROOT"], "sqlite-muninn_amd", "ext", "muninn"))
    return c
def dump(tag):
    for t, order in (("v_config", "key"), ("v_nodes", "id"), ("v_edges", "1,3,2")):
        cols = "rowid, *" if t == "v_config" else "id, level, deleted, hex(vector)" if t == "v_nodes" else "*"
        for r in c.execute(f"SELECT {cols} FROM {t} ORDER BY {order}"):
            print(tag, t, r)
c = connect()
X = np.random.default_rng(77).standard_normal((1400, 10), dtype=np.float32)
c.execute("CREATE VIRTUAL TABLE v USING hnsw_index(dimensions=10, metric='l2', m=3, ef_construction=24)")
ins = lambda i: c.execute("INSERT INTO v (rowid, vector) VALUES (?, ?)", (i + 1, X[i].tobytes()))
c.execute("BEGIN")
for i in range(0, 300): ins(i)
c.execute("COMMIT")
for i in range(300, 320): ins(i)                      # autocommit rows
dump("plain")
c.execute("BEGIN")
for i in range(320, 360): ins(i)
c.execute("ROLLBACK")                                 # 40 nodes stay in the index without shadow rows
c.execute("BEGIN")
for i in range(360, 450): ins(i)
dump("after-rollback")
for d in (3, 17, 250, 361, 400): c.execute("DELETE FROM v WHERE rowid = ?", (d,))
for i in range(450, 600): ins(i)
dump("after-deletes")
try:                                                  # a statement that fails half way inside a transaction: its rows roll back
    c.execute("INSERT INTO v (rowid, vector) SELECT 6000 + value, CASE WHEN value < 4 THEN zeroblob(40) ELSE x'00' END "
              "FROM (SELECT 1 AS value UNION ALL SELECT 2 UNION ALL SELECT 3 UNION ALL SELECT 4)")
except sqlite3.Error as e:
    print("failed:", e)
for i in range(600, 700): ins(i)
dump("after-failed-statement")
c.execute("SAVEPOINT a")
for i in range(700, 730): ins(i)
c.execute("ROLLBACK TO a")
c.execute("RELEASE a")
for i in range(730, 850): ins(i)
c.execute("COMMIT")
dump("after-savepoint")
c.close()
c = connect()                                         # reopen: lists in primary-key order, rolled-back nodes gone
for i in range(850, 1100): ins(i)
dump("after-reopen")
print(c.execute("SELECT rowid, distance FROM v WHERE vector MATCH ? AND k = 8 AND ef_search = 50", (X[7].tobytes(),)).fetchall())
"""
    import subprocess
    import sys

    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    return r.stdout.splitlines()


@pytest.mark.gpu
def test_edge_by_edge_persistence_leaves_the_tables_whole_node_rewrites_leave(ext_built, gpu, tmp_path):
    """Exact mode writes only the "{t}_edges" rows an insert changed (mn_hnsw_insert_logged) where the reference rewrites
    the new node and all its neighbours whole (src/hnsw_vtab.c:755-776).  MUNINN_HNSW_DELTA=0 is that whole-node rewrite
    (the path every reference-recorded golden was green on before the log existed): a session with m = 3 (prunes from the
    first rows on), autocommit rows, a ROLLBACK, DELETEs, statements failing half way inside a transaction, a SAVEPOINT
    rolled back and a reopen must leave the same _config (rowids included), _nodes and _edges, and answer alike."""
    a = _delta_session(ext_built, str(tmp_path / "a.db"), True)
    b = _delta_session(ext_built, str(tmp_path / "b.db"), False)
    assert len(a) > 20_000
    sa, sb = set(a), set(b)
    assert a == b, f"edge by edge only: {sorted(sa - sb)[:12]}; whole-node only: {sorted(sb - sa)[:12]}"
