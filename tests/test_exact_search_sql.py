"""hnsw_search_exact, the SQL face of the exact search (ext/mn_hnsw_tvf.c), and the three C-ABI symbols behind it.
The tests without the gpu mark run where no device exists: registration, schema, an error raised before any device call,
and the exported symbols."""
import os
import sqlite3
import subprocess

import numpy as np
import pytest

from util import gauss, ranks_within, same_bits, small_hnsw_table

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXT_DIR = os.path.join(ROOT, "sqlite-muninn_amd", "ext")
EXT = os.path.join(EXT_DIR, "muninn")
NEW_SYMBOLS = ("mn_hnsw_search_exact_batch", "mn_hnsw_search_exact_batch_dev", "mn_hnsw_last_exact")


@pytest.fixture
def cpu_conn(mn):
    """The extension loaded where no device exists: only statements that end before any device call may run here."""
    mn.build()
    subprocess.run(["make", "-s", "-C", EXT_DIR], check=True)
    c = sqlite3.connect(":memory:")
    c.enable_load_extension(True)
    c.load_extension(EXT)
    yield c
    c.close()


# ───────────────────────── CPU ─────────────────────────

def test_module_registered(cpu_conn):
    names = {r[0] for r in cpu_conn.execute("SELECT name FROM pragma_module_list")}
    assert {"hnsw_search_exact", "hnsw_search_batch", "hnsw_index"} <= names


def test_schema(cpu_conn):
    cols = cpu_conn.execute("SELECT name, type, hidden FROM pragma_table_xinfo('hnsw_search_exact')").fetchall()
    assert cols == [("query_idx", "INTEGER", 0), ("id", "INTEGER", 0), ("distance", "REAL", 0), ("tbl", "TEXT", 1),
                    ("queries", "BLOB", 1), ("k", "INTEGER", 1), ("allow", "BLOB", 1)]
    # hnsw_search_batch keeps its own
    old = [r[0] for r in cpu_conn.execute("SELECT name FROM pragma_table_xinfo('hnsw_search_batch')")]
    assert old == ["query_idx", "id", "distance", "tbl", "queries", "k", "ef_search"]


def test_unknown_table_fails_before_any_device_call(cpu_conn):
    q = np.zeros(4, np.float32).tobytes()
    with pytest.raises(sqlite3.OperationalError) as ei:
        cpu_conn.execute("SELECT * FROM hnsw_search_exact WHERE tbl='nope' AND queries=? AND k=5", (q,)).fetchall()
    assert str(ei.value) == "hnsw_search_exact: no hnsw_index table named 'nope'"
    # without its three arguments the function has nothing to answer
    assert cpu_conn.execute("SELECT * FROM hnsw_search_exact").fetchall() == []


def test_schema_of_hnsw_search_batch(cpu_conn):
    cols = cpu_conn.execute("SELECT name, type, hidden FROM pragma_table_xinfo('hnsw_search_batch')").fetchall()
    assert cols == [("query_idx", "INTEGER", 0), ("id", "INTEGER", 0), ("distance", "REAL", 0), ("tbl", "TEXT", 1),
                    ("queries", "BLOB", 1), ("k", "INTEGER", 1), ("ef_search", "INTEGER", 1)]


@pytest.mark.parametrize("fn", ["hnsw_search_batch", "hnsw_search_exact"])
def test_a_missing_required_argument_answers_nothing(cpu_conn, fn):
    """Not an error, even when tbl names no table: the function is never asked."""
    assert cpu_conn.execute(f"SELECT * FROM {fn} WHERE tbl='nope'").fetchall() == []
    assert cpu_conn.execute(f"SELECT * FROM {fn} WHERE tbl='nope' AND k=3").fetchall() == []


@pytest.mark.parametrize("fn", ["hnsw_search_batch", "hnsw_search_exact"])
def test_arguments_are_bound_by_column_not_by_their_place_in_the_text(cpu_conn, fn):
    q = np.zeros(4, np.float32).tobytes()
    with pytest.raises(sqlite3.OperationalError) as ei:
        cpu_conn.execute(f"SELECT * FROM {fn} WHERE k=3 AND queries=? AND tbl='nope'", (q,)).fetchall()
    assert str(ei.value) == f"{fn}: no hnsw_index table named 'nope'"


@pytest.mark.parametrize("fn", ["hnsw_search_batch", "hnsw_search_exact"])
def test_a_null_table_name_is_reported_as_the_empty_name(cpu_conn, fn):
    q = np.zeros(4, np.float32).tobytes()
    with pytest.raises(sqlite3.OperationalError) as ei:
        cpu_conn.execute(f"SELECT * FROM {fn} WHERE tbl=? AND queries=? AND k=3", (None, q)).fetchall()
    assert str(ei.value) == f"{fn}: no hnsw_index table named ''"


def test_library_exports_the_entry_points(mn):
    lib = mn.build()
    out = subprocess.run(["nm", "-D", "--defined-only", lib], check=True, capture_output=True, text=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    assert set(NEW_SYMBOLS) <= exported
    bound = {s[0] for s in mn.hnsw.SYMBOLS}
    assert set(NEW_SYMBOLS) <= bound
    L = mn.lib()
    for name in NEW_SYMBOLS:
        assert getattr(L, name).argtypes is not None
    assert L.mn_abi_version() == 2


# ───────────────────────── GPU ─────────────────────────

def rows_of(cur, nq):
    out = [[] for _ in range(nq)]
    for qi, i, d in cur:
        out[qi].append((i, np.float32(d)))
    return out


def same_rows(rows, ids, ds, cnt):
    for qi, r in enumerate(rows):
        assert [x[0] for x in r] == ids[qi, :cnt[qi]].tolist(), qi
        assert same_bits(np.array([x[1] for x in r], np.float32), ds[qi, :cnt[qi]]), qi


@pytest.mark.gpu
def test_tvf_equals_search_exact_batch(cpu_conn, gpu):
    c = cpu_conn
    n, dim, nq, k = 600, 32, 25, 10
    X, Q = gauss(n, dim, 61), gauss(nq, dim, 62)
    ids = np.arange(1, n + 1, dtype=np.int64)
    c.execute(f"CREATE VIRTUAL TABLE ev USING hnsw_index(dimensions={dim}, metric='l2', m=8, ef_construction=60)")
    g = gpu.HnswIndex(dim, "l2", 8, 60)
    with c:
        for i in range(n):
            c.execute("INSERT INTO ev (rowid, vector) VALUES (?, ?)", (int(ids[i]), X[i].tobytes()))
            assert g.insert(int(ids[i]), X[i]) == 0
    c.execute("DELETE FROM ev WHERE rowid = 17")
    assert g.delete(17) == 0
    sql = "SELECT query_idx, id, distance FROM hnsw_search_exact WHERE tbl='ev' AND queries=? AND k=?"
    same_rows(rows_of(c.execute(sql, (Q.tobytes(), k)), nq), *g.search_exact_batch(Q, k))
    allow = np.concatenate([ids[::3], [17, 10 ** 9]]).astype(np.int64)
    wi, wd, wc = g.search_exact_batch(Q, k, allow)
    assert (wi[wi >= 0] % 3 == 1).all()
    same_rows(rows_of(c.execute(sql + " AND allow=?", (Q.tobytes(), k, allow.tobytes())), nq), wi, wd, wc)
    assert c.execute(sql + " AND allow=?", (Q.tobytes(), k, b"")).fetchall() == []
    same_rows(rows_of(c.execute(sql + " AND allow=?", (Q.tobytes(), k, None)), nq), *g.search_exact_batch(Q, k))
    with pytest.raises(sqlite3.OperationalError, match=r"hnsw_search_exact: queries must be a multiple of 128 bytes \(32-dim f32\), got 3"):
        c.execute(sql, (b"123", k)).fetchall()
    with pytest.raises(sqlite3.OperationalError, match=r"hnsw_search_exact: allow must be a multiple of 8 bytes \(int64 rowids\), got 5"):
        c.execute(sql + " AND allow=?", (Q.tobytes(), k, b"12345")).fetchall()
    with pytest.raises(sqlite3.OperationalError, match="hnsw_search_exact: no hnsw_index table named 'nope'"):
        c.execute(sql.replace("'ev'", "'nope'"), (Q.tobytes(), k)).fetchall()
    g.close()


@pytest.mark.gpu
def test_rows_queued_in_the_open_transaction_are_found(mn, gpu, monkeypatch):
    monkeypatch.setenv("MUNINN_HNSW_MODE", "deferred")
    subprocess.run(["make", "-s", "-C", EXT_DIR], check=True)
    c = sqlite3.connect(":memory:")
    c.enable_load_extension(True)
    c.load_extension(EXT)
    c.isolation_level = None
    dim = 8
    X = gauss(40, dim, 71)
    c.execute(f"CREATE VIRTUAL TABLE dv USING hnsw_index(dimensions={dim}, metric='l2', m=4)")
    c.execute("BEGIN")
    for i in range(40):
        c.execute("INSERT INTO dv (rowid, vector) VALUES (?, ?)", (i + 1, X[i].tobytes()))
    rows = c.execute("SELECT query_idx, id, distance FROM hnsw_search_exact WHERE tbl='dv' AND queries=? AND k=1",
                     (X[[5, 39]].tobytes(),)).fetchall()
    assert rows == [(0, 6, 0.0), (1, 40, 0.0)]
    c.execute("COMMIT")
    c.close()


@pytest.mark.gpu
def test_rows_are_numbered_by_query_and_rank(cpu_conn, gpu):
    """rowid = query_idx * k + rank within the query, for both functions; a query with fewer than k rows leaves a gap in the
    numbering, a query with none is skipped, and an answer of empty groups only is no rows."""
    c = cpu_conn
    small_hnsw_table(c, "sv")
    Q, k = gauss(5, 8, 102).tobytes(), 3
    for fn in ("hnsw_search_batch", "hnsw_search_exact"):
        rows = c.execute(f"SELECT rowid, query_idx, id FROM {fn} WHERE tbl='sv' AND queries=? AND k=?", (Q, k)).fetchall()
        assert [r[1] for r in rows] == [qi for qi in range(5) for _ in range(k)], fn
        assert [r[0] for r in rows] == [r[1] * k + rank for r, rank in zip(rows, ranks_within(r[1] for r in rows))], fn
        assert not {7, 23} & {r[2] for r in rows}, fn
    sql = "SELECT rowid, query_idx, id FROM hnsw_search_exact WHERE tbl='sv' AND queries=? AND k=? AND allow=?"
    rows = c.execute(sql, (Q, k, np.array([3, 30], np.int64).tobytes())).fetchall()
    assert [r[1] for r in rows] == [qi for qi in range(5) for _ in range(2)]  # two rows a query: fewer than k
    assert [r[0] for r in rows] == [0, 1, 3, 4, 6, 7, 9, 10, 12, 13]
    assert all({r[2] for r in rows if r[1] == qi} == {3, 30} for qi in range(5))
    assert c.execute(sql, (Q, k, np.array([7], np.int64).tobytes())).fetchall() == []  # a deleted row: every group is empty
