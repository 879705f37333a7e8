"""muninn_extract_er and the four C-ABI entry points behind it, as far as they go where no device exists: registration, the
answers given before any device call, the exported and bound symbols, and every argument check of the C-ABI — each made on
the host before anything is launched."""
import ctypes as C
import os
import sqlite3
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXT_DIR = os.path.join(ROOT, "sqlite-muninn_amd", "ext")
NEW_SYMBOLS = ("mn_er_jaro_winkler", "mn_er_candidates", "mn_er_score", "mn_hnsw_er_edges")


@pytest.fixture
def cpu_conn(mn):
    mn.build()
    subprocess.run(["make", "-s", "-C", EXT_DIR], check=True)
    c = sqlite3.connect(":memory:")
    c.enable_load_extension(True)
    c.load_extension(os.path.join(EXT_DIR, "muninn"))
    yield c
    c.close()


def test_function_registered(cpu_conn):
    rows = cpu_conn.execute("SELECT name, narg FROM pragma_function_list WHERE name = 'muninn_extract_er'").fetchall()
    assert rows == [("muninn_extract_er", -1)]


def test_fewer_than_six_arguments_is_the_reference_message(cpu_conn):
    for sql in ("SELECT muninn_extract_er()", "SELECT muninn_extract_er('v', 'name', 5, 0.3, 0.5)"):
        with pytest.raises(sqlite3.OperationalError) as ei:
            cpu_conn.execute(sql).fetchall()
        assert str(ei.value) == "muninn_extract_er: requires at least 6 arguments"  # src/llama_er.c:115-118


def test_missing_entities_table_is_an_sql_error(cpu_conn):
    with pytest.raises(sqlite3.OperationalError, match="no such table: entities"):
        cpu_conn.execute("SELECT muninn_extract_er('v', 'name', 5, 0.3, 0.5, 0.0)").fetchall()
    cpu_conn.execute("CREATE TABLE entities(entity_id TEXT, name TEXT, source TEXT)")
    with pytest.raises(sqlite3.OperationalError, match="no such column: nope"):
        cpu_conn.execute("SELECT muninn_extract_er('v', 'nope', 5, 0.3, 0.5, 0.0)").fetchall()


def test_empty_entities_table_answers_before_the_index_is_touched(cpu_conn):
    cpu_conn.execute("CREATE TABLE entities(entity_id TEXT, name TEXT, source TEXT)")
    # no table 'v' exists: the answer comes before anything looks for it (src/llama_er.c:190-193)
    assert cpu_conn.execute("SELECT muninn_extract_er('v', 'name', 5, 0.3, 0.5, 0.0)").fetchall() == [('{"clusters":{}}',)]
    assert cpu_conn.execute("SELECT muninn_extract_er('v', 'name', 5, 0.3, 0.5, 0.0, NULL, 0.5, 'same_source')").fetchall() == \
        [('{"clusters":{}}',)]


def test_null_name_and_unknown_index_are_errors_before_any_device_call(cpu_conn):
    cpu_conn.execute("CREATE TABLE entities(entity_id TEXT, name TEXT, source TEXT)")
    cpu_conn.execute("INSERT INTO entities VALUES ('a', 'x', NULL)")
    with pytest.raises(sqlite3.OperationalError) as ei:
        cpu_conn.execute("SELECT muninn_extract_er('v', 'name', 5, 0.3, 0.5, 0.0)").fetchall()
    assert str(ei.value) == "muninn_extract_er: no hnsw_index table named 'v'"
    cpu_conn.execute("INSERT INTO entities VALUES ('b', NULL, 's')")
    with pytest.raises(sqlite3.OperationalError, match="entities row 2 has a NULL entity_id or name"):
        cpu_conn.execute("SELECT muninn_extract_er('v', 'name', 5, 0.3, 0.5, 0.0)").fetchall()


def test_library_exports_and_binds_the_entry_points(mn):
    lib = mn.build()
    out = subprocess.run(["nm", "-D", "--defined-only", lib], check=True, capture_output=True, text=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    assert set(NEW_SYMBOLS) <= exported
    assert set(NEW_SYMBOLS) == {s[0] for s in mn.hnsw.ER_SYMBOLS} <= {s[0] for s in mn.hnsw.SYMBOLS}
    L = mn.lib()
    for name in NEW_SYMBOLS:
        assert getattr(L, name).argtypes is not None
    assert L.mn_abi_version() == 2
    assert C.sizeof(mn.hnsw.ErEdge) == 16 and mn.er.EDGE_DTYPE.itemsize == 16


def err(mn):
    return mn.lib().mn_last_error().decode()


def names(mn, *raw):
    return mn.er.pack_names(raw)


def i32(*v):
    return np.array(v, np.int32)


def test_jaro_winkler_argument_checks(mn):
    L = mn.lib()
    arena, off = names(mn, b"abc", b"abd")
    out = np.zeros(4, np.float64)
    assert L.mn_er_jaro_winkler(0, arena, off, 2, i32(0), i32(0), 0, out) == 0  # nothing to do is no error
    for a, b in ((2, 0), (0, -1)):
        assert L.mn_er_jaro_winkler(1, arena, off, 2, i32(a), i32(b), 0, out) == -1
        assert err(mn) == "mn_er_jaro_winkler: pair 0 names a string outside [0, 2)"
    bad = off.copy()
    bad[1] = 7
    assert L.mn_er_jaro_winkler(1, arena, bad, 2, i32(0), i32(1), 0, out) == -1
    assert err(mn) == "mn_er_jaro_winkler: name offsets are not monotone at name 1"
    bad = off.copy() - 1
    assert L.mn_er_jaro_winkler(1, arena, bad, 2, i32(0), i32(1), 0, out) == -1
    assert err(mn) == "mn_er_jaro_winkler: name offsets must start at or after 0 (got -1)"
    arena, off = names(mn, b"x" * 4097, b"y")
    assert L.mn_er_jaro_winkler(1, arena, off, 2, i32(0), i32(1), 0, out) == -1
    assert err(mn) == "mn_er_jaro_winkler: name 0 is 4097 bytes long, more than the 4096 this library stages"


def test_candidates_argument_checks(mn):
    L = mn.lib()
    ent = np.array([1, 2], np.int64)
    ids = np.zeros((2, 1), np.int64)
    ds = np.zeros((2, 1), np.float32)
    cnt = np.zeros(2, np.int32)
    r1, r2, d = np.zeros(2, np.int32), np.zeros(2, np.int32), np.zeros(2, np.float64)
    assert L.mn_er_candidates(0, 1, ent, ids, ds, cnt, 0.5, 0, r1, r2, d) == 0
    assert L.mn_er_candidates(2, 0, ent, ids, ds, cnt, 0.5, 0, r1, r2, d) == -1
    assert err(mn) == "mn_er_candidates: kk must be >= 1 (got 0)"
    assert L.mn_er_candidates(2, 1, ent, ids, ds, cnt, float("nan"), 0, r1, r2, d) == -1
    assert err(mn) == "mn_er_candidates: dist_threshold is NaN"
    assert L.mn_er_candidates(-1, 1, ent, ids, ds, cnt, 0.5, 0, r1, r2, d) == -1
    assert err(mn) == "mn_er_candidates: bad arguments"


def test_score_argument_checks(mn):
    L = mn.lib()
    arena, off = names(mn, b"abc", b"abd")
    edges = np.zeros(2, mn.er.EDGE_DTYPE)
    d = np.zeros(1, np.float64)

    def call(r1=0, r2=1, off_=off, arena_=arena, guard=0, w=0.5, thr=0.5, n_cand=1):
        return L.mn_er_score(n_cand, i32(r1), i32(r2), d, 2, arena_, off_, None, guard, w, thr, 0, edges.ctypes.data)

    assert call(n_cand=0) == 0
    assert call(r2=2) == -1 and err(mn) == "mn_er_score: candidate 0 names an entity outside [0, 2)"
    assert call(r1=-1) == -1 and err(mn) == "mn_er_score: candidate 0 names an entity outside [0, 2)"
    assert call(guard=3) == -1 and err(mn) == "mn_er_score: unknown type guard 3"
    assert call(w=float("nan")) == -1 and err(mn) == "mn_er_score: jw_weight is NaN"
    assert call(thr=float("nan")) == -1 and err(mn) == "mn_er_score: match_threshold is NaN"
    bad = off.copy()
    bad[2] = 1
    assert call(off_=bad) == -1 and err(mn) == "mn_er_score: name offsets are not monotone at name 1"
    big_arena, big_off = names(mn, b"x" * 5000, b"y")
    assert call(off_=big_off, arena_=big_arena) == -1
    assert err(mn) == "mn_er_score: name 0 is 5000 bytes long, more than the 4096 this library stages"


def test_er_edges_argument_checks(mn):
    """every check is made before the index is looked at: no index is needed to see them"""
    L = mn.lib()
    arena, off = names(mn, b"abc", b"abd")
    ent = np.array([1, 2], np.int64)
    edges = np.zeros(2 * 128, mn.er.EDGE_DTYPE)

    def call(k=3, thr=0.3, w=0.5, mt=0.7, guard=0, blocking=0, off_=off, arena_=arena):
        return L.mn_hnsw_er_edges(None, 2, ent, arena_, off_, None, k, thr, w, mt, guard, blocking, edges.ctypes.data, None)

    for k in (0, 128, -5):
        assert call(k=k) == -1
        assert err(mn).startswith(f"mn_hnsw_er_edges: k must be 1..127 (got {k})")
    assert call(blocking=2) == -1 and err(mn) == "mn_hnsw_er_edges: unknown blocking 2"
    assert call(thr=float("nan")) == -1 and err(mn) == "mn_hnsw_er_edges: dist_threshold is NaN"
    assert call(w=float("nan")) == -1 and err(mn) == "mn_hnsw_er_edges: jw_weight is NaN"
    assert call(mt=float("nan")) == -1 and err(mn) == "mn_hnsw_er_edges: match_threshold is NaN"
    assert call(guard=-1) == -1 and err(mn) == "mn_hnsw_er_edges: unknown type guard -1"
    big_arena, big_off = names(mn, b"x" * 4097, b"y")
    assert call(off_=big_off, arena_=big_arena) == -1
    assert err(mn) == "mn_hnsw_er_edges: name 0 is 4097 bytes long, more than the 4096 this library stages"
    assert call(k=127) == -1 and err(mn) == "mn_hnsw_er_edges: no index"  # all arguments in order: only now the index matters


def test_result_subtype_slot_matches_a_real_sqlite_header():
    """ext/mn_er_sql.c hard-codes the slot of sqlite3_result_subtype in sqlite3_api_routines; scripts/gen_er_golden.py measured
    it on a genuine sqlite3ext.h (the way tests/golden/sqlite_abi.json was measured for mn_sqlite_abi.h's slots)"""
    import gzip
    import json
    import re

    with gzip.open(os.path.join(ROOT, "tests", "golden", "er.json.gz"), "rb") as f:
        want = json.loads(f.read())["sqlite_slots"]
    src = open(os.path.join(EXT_DIR, "mn_er_sql.c")).read()
    got = {k: int(v) for k, v in re.findall(r"#define MN_ER_SLOT_(\w+) (\d+)", src)}
    assert got == want == {"result_subtype": 209}
    hdr = open(os.path.join(EXT_DIR, "mn_sqlite_abi.h")).read()
    assert int(re.search(r"void \*slot\[(\d+)\]", hdr).group(1)) > got["result_subtype"]  # inside the declared table
    assert "sqlite3_libversion_number() >= 3009000" in src  # the routine exists since 3.9.0: checked where it is called
