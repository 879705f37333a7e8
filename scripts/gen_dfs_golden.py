"""Writes tests/golden/dfs.json.gz: what the REFERENCE's graph_dfs returns (oracle/_ref/muninn.so through sqlite3) for the
cases and queries of tests/test_bfs_model.py and the statements of tests/test_dfs_sql.py.  Runs only where the compiled
reference exists; the tests read the file.  Recorded rows and error strings only.

    python scripts/gen_dfs_golden.py
"""
import gzip
import json
import os
import sqlite3
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import test_bfs_model as tb  # noqa: E402
import test_dfs_model as tm  # noqa: E402
import test_dfs_sql as ts  # noqa: E402
from oracle import orc_graph as og  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "dfs.json.gz")


def ref_conn():
    c = sqlite3.connect(":memory:")
    c.enable_load_extension(True)
    c.load_extension(og.REF_EXT_SO[:-3])
    return c


def main():
    assert og.have_ref_graph(), "oracle/_ref/muninn.so is not built"
    out = {"dfs": {}, "sql": {}}
    c = ref_conn()
    for name, rows in sorted(tb.graph_cases().items()):
        kind = "INTEGER" if name == "integers" else "TEXT"
        c.execute(f"CREATE TABLE t_{name}(s {kind}, d {kind})")
        c.executemany(f"INSERT INTO t_{name} VALUES (?, ?)", rows)
        out["dfs"][name] = [
            [list(r) for r in c.execute(f"SELECT node, depth, parent FROM graph_dfs('t_{name}', 's', 'd', ?, ?, ?)", q).fetchall()]
            for q in tb.bfs_queries()[name]]
    c.close()
    c = ref_conn()
    ts.fill_tables(c)
    for name, sql in sorted({**ts.HOST_STATEMENTS, **ts.DEVICE_STATEMENTS}.items()):
        out["sql"][name] = ts.answer(c, sql)
        print(name, "→", out["sql"][name].get("error") or f"{len(out['sql'][name]['rows'])} rows")
    c.close()
    # the grid must be able to tell a depth-first traversal from a breadth-first one, and a wrong depth rule from the right one
    order, fewer, deeper, both = tm.non_vacuity(out["dfs"])
    assert order > 0, "no traversal's node order differs from BFS's"
    assert fewer > 0, "no depth-limited traversal returns fewer rows than BFS at the same limit"
    assert deeper > 0, "no node is recorded deeper than its BFS depth"
    assert both > 0, "no 'both' case differs from 'forward'"
    with gzip.GzipFile(OUT, "wb", 9, mtime=0) as f:
        f.write(json.dumps(out, separators=(",", ":")).encode())
    print(os.path.relpath(OUT, ROOT), os.path.getsize(OUT), "bytes;", sum(len(v) for v in out["dfs"].values()), "traversals;",
          order, "in another order than BFS,", fewer, "with fewer rows under a depth limit,", deeper, "with a node deeper than its BFS depth,",
          both, "'both' answers that differ from 'forward'")


if __name__ == "__main__":
    main()
