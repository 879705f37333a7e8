"""graph_shortest_path through the SQLite extension against what the compiled reference returned for the same statements
(tests/golden/shortest_path.json.gz, key "sql"; written by scripts/gen_sp_golden.py): schema, the positional mapping of the
hidden columns, the NULL weight column, the two error strings, rows with rowid = position.  Every comparison is equality of
whole rows (a REAL as the hex text of its f64) or of the error's text, under MUNINN_GRAPH_MODE=exact and =auto."""
import os
import sqlite3
import subprocess

import pytest

from test_sp_model import golden, graph_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXT = os.path.join(ROOT, "sqlite-muninn_amd", "ext", "muninn")

E = "edge_table='e' AND src_col='s' AND dst_col='d'"
F = "graph_shortest_path"

# statements that touch no device: errors, start == end, and names the table does not hold
HOST_STATEMENTS = {
    "no_arguments": f"SELECT * FROM {F}",
    "missing_end": f"SELECT * FROM {F}('e', 's', 'd', 'a')",
    "bad_identifier": f"SELECT * FROM {F}('e; drop', 's', 'd', 'a', 'd')",
    "bad_weight_identifier": f"SELECT * FROM {F}('e', 's', 'd', 'a', 'd', 'w; drop')",
    "missing_table": f"SELECT * FROM {F}('nope', 's', 'd', 'a', 'd', 'w')",
    "missing_table_unweighted": f"SELECT * FROM {F}('nope', 's', 'd', 'a', 'd')",
    "missing_start": f"SELECT rowid, * FROM {F}('e', 's', 'd', 'nowhere', 'd', 'w')",
    "missing_end_node": f"SELECT rowid, * FROM {F}('e', 's', 'd', 'a', 'nowhere', 'w')",
    "start_is_end_for_an_absent_name": f"SELECT rowid, * FROM {F}('e', 's', 'd', 'nowhere', 'nowhere', 'w')",
    "start_is_end_unweighted": f"SELECT rowid, * FROM {F}('e', 's', 'd', 'b', 'b')",
    "start_is_end_in_an_empty_table": f"SELECT rowid, * FROM {F}('empty', 's', 'd', 'a', 'a', 'w')",
    "empty_table": f"SELECT rowid, * FROM {F}('empty', 's', 'd', 'a', 'b', 'w')",
    # xFilter maps by position: the fifth constraint is weight_col, and its value lands in end_node — no node is called 'w'
    "weight_col_as_fifth_constraint": f"SELECT rowid, * FROM {F} WHERE {E} AND start_node='a' AND weight_col='w'",
}

DEVICE_STATEMENTS = {
    "all_six": f"SELECT rowid, * FROM {F} WHERE {E} AND start_node='a' AND end_node='f' AND weight_col='w'",
    "all_six_function_form": f"SELECT rowid, node, distance, path_order FROM {F}('e', 's', 'd', 'a', 'd', 'w')",
    "five_unweighted": f"SELECT rowid, * FROM {F}('e', 's', 'd', 'a', 'f')",
    "null_weight_col": f"SELECT rowid, * FROM {F}('e', 's', 'd', 'a', 'f', NULL)",
    "hidden_columns": f"SELECT node, edge_table, src_col, dst_col, start_node, end_node, weight_col FROM {F}('e', 's', 'd', 'a', 'e', 'w')",
    "typeof": f"SELECT typeof(node), typeof(distance), typeof(path_order) FROM {F}('ei', 's', 'd', '7', '10', 'w')",
    "integer_columns": f"SELECT rowid, * FROM {F}('ei', 's', 'd', '7', '10', 'w')",
    "integer_columns_unweighted": f"SELECT rowid, * FROM {F}('ei', 's', 'd', '7', '10')",
    "weights_as_text_and_null": f"SELECT rowid, * FROM {F}('et', 's', 'd', 'a', 'e', 'w')",
    # SQLite reads a double-quoted name that is no column as a string: the statement compiles and every weight reads 0.0
    "missing_weight_column": f"SELECT rowid, * FROM {F}('e', 's', 'd', 'a', 'd', 'nope')",
    "no_way": f"SELECT rowid, * FROM {F}('e', 's', 'd', 'f', 'a', 'w')",
    "zero_cycle": f"SELECT rowid, * FROM {F}('z', 's', 'd', 's', 't', 'w')",
    "ties_forty_nodes": f"SELECT rowid, * FROM {F}('ties', 's', 'd', 'n5', 'n20', 'w')",
    "infinite_weights": f"SELECT rowid, * FROM {F}('inf', 's', 'd', 'n3', 'n0', 'w')",
    "filtered_and_ordered": f"SELECT node, distance FROM {F}('ties', 's', 'd', 'n1', 'n19', 'w') WHERE distance > 0 ORDER BY path_order DESC",
    "weight_column_is_the_destination": f"SELECT rowid, * FROM {F}('ei', 's', 'd', '1', '2', 'd')",
}


def fill_tables(c):
    """the tables the statements read; also what scripts/gen_sp_golden.py gives the reference"""
    cases = graph_cases()
    for name, rows in (("e", cases["negative"]), ("z", cases["zero_cycle"]), ("ties", cases["ties"]), ("inf", cases["infinite"])):
        c.execute(f"CREATE TABLE {name}(s TEXT, d TEXT, w REAL)")
        c.executemany(f"INSERT INTO {name} VALUES (?, ?, ?)", rows)
    c.execute("CREATE TABLE ei(s INTEGER, d INTEGER, w REAL)")
    c.executemany("INSERT INTO ei VALUES (?, ?, ?)", [(1, 2, 4.0), (1, 3, 1.5), (3, 2, 2.0), (2, 10, 1.0), (10, 1, 1.0), (7, 1, 0.25)])
    c.execute("CREATE TABLE et(s TEXT, d TEXT, w)")  # sqlite3_column_double: '2.5' reads 2.5, 'heavy' and NULL read 0.0
    c.executemany("INSERT INTO et VALUES (?, ?, ?)", [("a", "b", "2.5"), ("a", "c", "heavy"), ("c", "d", None), ("b", "e", 1),
                                                      ("d", "e", "3e0"), ("a", "e", " 3.25")])
    c.execute("CREATE TABLE empty(s TEXT, d TEXT, w REAL)")
    c.commit()


def answer(c, sql):
    """what a statement gives: its rows, or its error's text"""
    try:
        return {"rows": [[v.hex() if isinstance(v, float) else v for v in r] for r in c.execute(sql).fetchall()]}
    except sqlite3.OperationalError as e:
        return {"error": str(e)}


@pytest.fixture
def conn(mn):
    mn.build()
    subprocess.run(["make", "-s", "-C", os.path.dirname(EXT)], check=True)
    c = sqlite3.connect(":memory:")
    c.enable_load_extension(True)
    c.load_extension(EXT)
    fill_tables(c)
    yield c
    c.close()


def test_extension_registers_graph_shortest_path_with_the_reference_schema(conn):
    names = {r[0] for r in conn.execute("SELECT name FROM pragma_module_list")}
    assert {"graph_shortest_path", "graph_bfs", "graph_select"} <= names
    cols = [[r[1], r[2], r[6]] for r in conn.execute("SELECT * FROM pragma_table_xinfo('graph_shortest_path')")]
    assert cols == golden()["schema"]
    assert [c[0] for c in cols] == ["node", "distance", "path_order", "edge_table", "src_col", "dst_col", "start_node", "end_node",
                                    "weight_col"]


@pytest.mark.parametrize("mode", ["exact", "auto"])
@pytest.mark.parametrize("name", sorted(HOST_STATEMENTS))
def test_statements_that_need_no_device(conn, monkeypatch, name, mode):
    monkeypatch.setenv("MUNINN_GRAPH_MODE", mode)
    want = golden()["sql"][name]
    assert answer(conn, HOST_STATEMENTS[name]) == want, name
    if name in ("no_arguments", "missing_end"):
        assert want == {"error": "graph_shortest_path: requires edge_table, src_col, dst_col, start_node, end_node"}
    if name in ("bad_identifier", "bad_weight_identifier", "missing_table", "missing_table_unweighted"):
        assert want == {"error": "graph_shortest_path: search failed"}
    if name == "start_is_end_for_an_absent_name":
        assert want == {"rows": [[0, "nowhere", (0.0).hex(), 0]]}
    if name in ("missing_start", "missing_end_node", "empty_table", "weight_col_as_fifth_constraint"):
        assert want == {"rows": []}


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["exact", "auto"])
@pytest.mark.parametrize("name", sorted(DEVICE_STATEMENTS))
def test_statements_row_for_row(gpu, conn, monkeypatch, name, mode):
    monkeypatch.setenv("MUNINN_GRAPH_MODE", mode)
    want = golden()["sql"][name]
    assert "rows" in want and (len(want["rows"]) >= 1 or name == "no_way")
    assert answer(conn, DEVICE_STATEMENTS[name]) == want, name


@pytest.mark.gpu
def test_every_recorded_path_through_sql(gpu, conn):
    """the cases of tests/test_sp_model.py, one table each, every recorded (start, end)"""
    from test_sp_model import path_queries

    z = golden()["paths"]
    for name, rows in sorted(graph_cases().items()):
        conn.execute(f"CREATE TABLE t_{name}(s TEXT, d TEXT, w REAL)")
        conn.executemany(f"INSERT INTO t_{name} VALUES (?, ?, ?)", rows)
        for (start, end), want in zip(path_queries()[name], z[name]):
            got = conn.execute(f"SELECT node, distance, path_order FROM {F}('t_{name}', 's', 'd', ?, ?, 'w')", (start, end)).fetchall()
            assert [r[2] for r in got] == list(range(len(got)))
            assert [[r[0], r[1].hex()] for r in got] == want, (name, start, end)
