"""Writes tests/golden/bfs.json.gz: what the REFERENCE's graph_bfs and graph_shortest_path return (oracle/_ref/muninn.so
through sqlite3) for the cases of tests/test_bfs_model.py and the statements of tests/test_bfs_sql.py.  Runs only where the
compiled reference exists; the tests read the file.  Recorded rows only.

    python scripts/gen_bfs_golden.py
"""
import gzip
import json
import os
import sqlite3
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import test_bfs_model as tm  # noqa: E402
import test_bfs_sql as ts  # noqa: E402
from oracle import orc_graph as og  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "bfs.json.gz")


def ref_conn():
    c = sqlite3.connect(":memory:")
    c.enable_load_extension(True)
    c.load_extension(og.REF_EXT_SO[:-3])
    return c


def main():
    assert og.have_ref_graph(), "oracle/_ref/muninn.so is not built"
    out = {"bfs": {}, "paths": {}, "sql": {}}
    c = ref_conn()
    for name, rows in sorted(tm.graph_cases().items()):
        kind = "INTEGER" if name == "integers" else "TEXT"
        c.execute(f"CREATE TABLE t_{name}(s {kind}, d {kind})")
        c.executemany(f"INSERT INTO t_{name} VALUES (?, ?)", rows)
        out["bfs"][name] = [
            [list(r) for r in c.execute(f"SELECT node, depth, parent FROM graph_bfs('t_{name}', 's', 'd', ?, ?, ?)", q).fetchall()]
            for q in tm.bfs_queries()[name]]
        out["paths"][name] = []
        for q in tm.path_queries()[name]:
            got = c.execute(f"SELECT node, distance, path_order FROM graph_shortest_path('t_{name}', 's', 'd', ?, ?) "
                            f"ORDER BY path_order", q).fetchall()
            assert [r[2] for r in got] == list(range(len(got))) and all(r[1] == r[2] for r in got)
            out["paths"][name].append([r[0] for r in got])
    c.close()
    c = ref_conn()
    ts.fill_tables(c)
    for name, sql in sorted({**ts.HOST_STATEMENTS, **ts.DEVICE_STATEMENTS}.items()):
        out["sql"][name] = ts.answer(c, sql)
        print(name, "→", out["sql"][name].get("error") or f"{len(out['sql'][name]['rows'])} rows")
    c.close()
    # the grid must be able to tell a wrong traversal from a right one
    every = [(name, q, rows) for name in out["bfs"] for q, rows in zip(tm.bfs_queries()[name], out["bfs"][name])]
    assert any(max(r[1] for r in rows) >= 3 for _, _, rows in every), "no case has three levels"
    two_parents = 0
    for name, (start, max_depth, direction), rows in every:
        if direction != "forward" or max_depth < 100:
            continue
        at = {r[0]: r[1] for r in rows}
        for r in rows:
            others = {str(s) for s, d in tm.graph_cases()[name]
                      if str(d) == r[0] and str(s) != r[2] and str(s) != r[0] and at.get(str(s)) == r[1] - 1}
            two_parents += bool(r[2] is not None and others)
    assert two_parents > 0, "no node is reachable through two parents of the same level"
    by_query = {(name, q[0], q[1], q[2]): rows for name, q, rows in every}
    assert any(rows != by_query.get((name, s, m, "forward")) for (name, s, m, d), rows in by_query.items() if d == "both"), \
        "no 'both' case differs from 'forward'"
    assert all(len(p) == 0 or p[0] == q[0] for name in out["paths"] for q, p in zip(tm.path_queries()[name], out["paths"][name]))
    with gzip.GzipFile(OUT, "wb", 9, mtime=0) as f:
        f.write(json.dumps(out, separators=(",", ":")).encode())
    print(os.path.relpath(OUT, ROOT), os.path.getsize(OUT), "bytes;", len(every), "traversals,", two_parents,
          "nodes with a second parent,", sum(len(v) for v in out["paths"].values()), "paths")


if __name__ == "__main__":
    main()
