"""graph_dfs through the SQLite extension against what the compiled reference returned for the same statements
(tests/golden/dfs.json.gz, key "sql"; written by scripts/gen_dfs_golden.py): schema, the positional mapping of the hidden
columns, defaults, error strings under the function's own name, rows in the stack's pop order.  Every comparison is equality
of whole rows."""
import os
import sqlite3

import pytest

from test_bfs_model import bfs_queries, graph_cases
from test_bfs_sql import big_rows
from test_dfs_model import golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXT = os.path.join(ROOT, "sqlite-muninn_amd", "ext", "muninn")

E = "edge_table='e' AND src_col='s' AND dst_col='d'"

# statements that touch no device: errors, answers that are the start row alone, the schema and the plan
HOST_STATEMENTS = {
    "bad_identifier": "SELECT * FROM graph_dfs WHERE edge_table='e; drop' AND src_col='s' AND dst_col='d' AND start_node='a'",
    "missing_table": "SELECT * FROM graph_dfs WHERE edge_table='nope' AND src_col='s' AND dst_col='d' AND start_node='a'",
    "missing_parameter": f"SELECT * FROM graph_dfs WHERE {E}",
    "no_arguments": "SELECT * FROM graph_dfs",
    "empty_table": "SELECT rowid, * FROM graph_dfs WHERE edge_table='empty' AND src_col='s' AND dst_col='d' AND start_node='a'",
    "max_depth_0": f"SELECT rowid, * FROM graph_dfs WHERE {E} AND start_node='a' AND max_depth=0",
    "max_depth_negative": f"SELECT rowid, * FROM graph_dfs WHERE {E} AND start_node='a' AND max_depth=-3 AND direction='both'",
    "unknown_direction": f"SELECT rowid, * FROM graph_dfs WHERE {E} AND start_node='a' AND max_depth=100 AND direction='sideways'",
    # xFilter maps by position: the string lands in max_depth, reads as 0, and the direction stays 'forward'
    "direction_without_max_depth": f"SELECT rowid, * FROM graph_dfs WHERE {E} AND start_node='a' AND direction='both'",
    "schema": "SELECT cid, name, type, \"notnull\", dflt_value, pk, hidden FROM pragma_table_xinfo('graph_dfs')",
    "query_plan": f"EXPLAIN QUERY PLAN SELECT * FROM graph_dfs WHERE {E} AND start_node='a' AND max_depth=3 AND direction='both'",
}

DEVICE_STATEMENTS = {
    "all_six_both": f"SELECT rowid, * FROM graph_dfs WHERE {E} AND start_node='a' AND max_depth=100 AND direction='both'",
    "all_six_forward": f"SELECT rowid, * FROM graph_dfs WHERE {E} AND start_node='a' AND max_depth=100 AND direction='forward'",
    "all_six_function_form": "SELECT rowid, node, depth, parent FROM graph_dfs('e', 's', 'd', 'a', 100, 'reverse')",
    "hidden_columns": f"SELECT node, edge_table, src_col, dst_col, start_node, max_depth, direction FROM graph_dfs "
                      f"WHERE {E} AND start_node='a' AND max_depth=1 AND direction='forward'",
    "max_depth_omitted": "SELECT rowid, * FROM graph_dfs('e', 's', 'd', 'a')",
    "direction_omitted": f"SELECT rowid, * FROM graph_dfs WHERE {E} AND start_node='a' AND max_depth=1",
    "both_omitted": f"SELECT rowid, * FROM graph_dfs WHERE {E} AND start_node='d'",
    "max_depth_2_both": f"SELECT rowid, * FROM graph_dfs WHERE {E} AND start_node='e' AND max_depth=2 AND direction='both'",
    "absent_start": f"SELECT rowid, * FROM graph_dfs WHERE {E} AND start_node='nowhere' AND max_depth=100 AND direction='both'",
    "integer_columns": "SELECT rowid, * FROM graph_dfs('ei', 's', 'd', '1', 100, 'both')",
    "integer_columns_typeof": "SELECT typeof(node), typeof(depth), typeof(parent) FROM graph_dfs('ei', 's', 'd', '7', 100, 'forward')",
    # rows with a NULL endpoint, in the directions whose statements never read them ("WHERE s = ?" matches no NULL)
    "null_source_forward": "SELECT rowid, * FROM graph_dfs('en', 's', 'd', 'a', 100, 'forward')",
    "null_target_reverse": "SELECT rowid, * FROM graph_dfs('er', 's', 'd', 'b', 100, 'reverse')",
    "table_2000_rows": "SELECT rowid, * FROM graph_dfs('big', 'src', 'dst', 'n0', 100, 'both')",
    "table_2000_rows_forward": "SELECT rowid, * FROM graph_dfs('big', 'src', 'dst', 'n3', 3, 'forward')",
    "filtered_and_ordered": f"SELECT node, depth FROM graph_dfs WHERE {E} AND start_node='a' AND max_depth=100 AND direction='both' "
                            f"AND depth = 1 ORDER BY node",
}


def fill_tables(c):
    """the tables the statements read; also what scripts/gen_dfs_golden.py gives the reference"""
    c.execute("CREATE TABLE e(s TEXT, d TEXT)")
    c.executemany("INSERT INTO e VALUES (?, ?)", graph_cases()["table"])
    c.execute("CREATE TABLE ei(s INTEGER, d INTEGER)")
    c.executemany("INSERT INTO ei VALUES (?, ?)", graph_cases()["integers"])
    c.execute("CREATE TABLE en(s TEXT, d TEXT)")
    c.executemany("INSERT INTO en VALUES (?, ?)", [("a", "b"), (None, "c"), ("a", "c"), ("b", "c"), (None, "a"), ("c", "d"), ("d", "a")])
    c.execute("CREATE TABLE er(s TEXT, d TEXT)")
    c.executemany("INSERT INTO er VALUES (?, ?)", [("a", "b"), ("b", None), ("c", "b"), ("d", "a"), ("c", None), ("d", "c"), ("b", "d")])
    c.execute("CREATE TABLE empty(s TEXT, d TEXT)")
    c.execute("CREATE TABLE big(src TEXT, dst TEXT)")
    c.executemany("INSERT INTO big VALUES (?, ?)", big_rows())
    c.commit()


def answer(c, sql):
    """what a statement gives: its rows, or its error's text"""
    try:
        return {"rows": [list(r) for r in c.execute(sql).fetchall()]}
    except sqlite3.OperationalError as e:
        return {"error": str(e)}


def _connect():
    import subprocess

    subprocess.run(["make", "-s", "-C", os.path.dirname(EXT)], check=True)
    c = sqlite3.connect(":memory:")
    c.enable_load_extension(True)
    c.load_extension(EXT)
    return c


@pytest.fixture
def conn(mn):
    mn.build()
    c = _connect()
    fill_tables(c)
    yield c
    c.close()


def test_extension_registers_graph_dfs(conn):
    names = {r[0] for r in conn.execute("SELECT name FROM pragma_module_list")}
    assert {"graph_dfs", "graph_bfs", "graph_shortest_path", "graph_degree"} <= names


def test_schema_equals_the_recorded_one(conn):
    want = golden()["sql"]["schema"]
    assert answer(conn, HOST_STATEMENTS["schema"]) == want
    assert [r[1] for r in want["rows"]] == ["node", "depth", "parent", "edge_table", "src_col", "dst_col", "start_node", "max_depth",
                                             "direction"]
    assert [r[6] for r in want["rows"]] == [0, 0, 0, 1, 1, 1, 1, 1, 1]


@pytest.mark.parametrize("name", sorted(HOST_STATEMENTS))
def test_statements_that_need_no_device(conn, name):
    want = golden()["sql"][name]
    assert answer(conn, HOST_STATEMENTS[name]) == want, name
    if name in ("bad_identifier", "missing_table"):
        assert want == {"error": "graph_dfs: traversal failed (check table/column names exist)"}
    if name in ("missing_parameter", "no_arguments"):
        assert want == {"error": "graph_dfs: requires edge_table, src_col, dst_col, start_node parameters"}
    if name in ("empty_table", "max_depth_0", "max_depth_negative", "unknown_direction", "direction_without_max_depth"):
        assert want == {"rows": [[0, "a", 0, None]]}


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(DEVICE_STATEMENTS))
def test_statements_row_for_row(gpu, conn, name):
    want = golden()["sql"][name]
    assert "rows" in want and len(want["rows"]) >= 1
    assert answer(conn, DEVICE_STATEMENTS[name]) == want, name


@pytest.mark.gpu
def test_every_recorded_traversal_through_sql(gpu, mn):
    """the cases of tests/test_bfs_model.py, one table each, every recorded (start, max_depth, direction)"""
    c = _connect()
    z = golden()["dfs"]
    for name, rows in sorted(graph_cases().items()):
        kind = "INTEGER" if name == "integers" else "TEXT"
        c.execute(f"CREATE TABLE t_{name}(s {kind}, d {kind})")
        c.executemany(f"INSERT INTO t_{name} VALUES (?, ?)", rows)
        for (start, max_depth, direction), want in zip(bfs_queries()[name], z[name]):
            got = c.execute(f"SELECT node, depth, parent FROM graph_dfs('t_{name}', 's', 'd', ?, ?, ?)", (start, max_depth, direction))
            assert [list(r) for r in got.fetchall()] == want, (name, start, max_depth, direction)
    c.close()


@pytest.mark.gpu
def test_graph_dfs_joins_graph_degree(gpu, conn):
    """a depth-first walk with each member's degree, in one statement"""
    got = conn.execute("SELECT b.node, b.depth, g.degree FROM graph_dfs('e', 's', 'd', 'a', 2, 'forward') AS b "
                       "JOIN graph_degree AS g ON g.node = b.node "
                       "WHERE g.edge_table = 'e' AND g.src_col = 's' AND g.dst_col = 'd' ORDER BY b.rowid").fetchall()
    dfs = conn.execute("SELECT node, depth FROM graph_dfs('e', 's', 'd', 'a', 2, 'forward')").fetchall()
    deg = dict(conn.execute(f"SELECT node, degree FROM graph_degree WHERE {E}").fetchall())
    # a's out-list is c, b, b, a: the last-listed unvisited entry goes first, so d is found under b and not under c
    assert dfs == [("a", 0), ("b", 1), ("d", 2), ("c", 1), ("e", 2)]
    assert got == [(n, d, deg[n]) for n, d in dfs]
