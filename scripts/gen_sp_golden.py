"""Writes tests/golden/shortest_path.json.gz: what the REFERENCE's graph_shortest_path returns (oracle/_ref/muninn.so through
sqlite3) with a weight column for the cases of tests/test_sp_model.py, and for the statements of
tests/test_shortest_path_sql.py.  Runs only where the compiled reference exists; the tests read the file.  Recorded data
only: node lists, f64 distances as hex text, error texts, the declared schema.

    python scripts/gen_sp_golden.py
"""
import gzip
import json
import os
import sqlite3
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import sp_model as sm  # noqa: E402
import test_shortest_path_sql as ts  # noqa: E402
import test_sp_model as tm  # noqa: E402
from oracle import orc_graph as og  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "shortest_path.json.gz")


def ref_conn():
    c = sqlite3.connect(":memory:")
    c.enable_load_extension(True)
    c.load_extension(og.REF_EXT_SO[:-3])
    return c


def ambiguous(rows, start, path):
    """whether some node of the recorded path has a second tight predecessor: another way to it, so another node list"""
    ids, index, out = sm.text_graph(rows)
    if len(path) < 2 or any(w < 0 for _, _, w in rows):
        return False
    dist = sm.distances(out, index[start])
    pred = sm.tight_predecessors(out, dist)
    return any(pred[index[v]] - {index[u]} for u, v in zip(path, path[1:]))


def main():
    assert og.have_ref_graph(), "oracle/_ref/muninn.so is not built"
    out = {"paths": {}, "sql": {}}
    c = ref_conn()
    n_ambiguous = 0
    for name, rows in sorted(tm.graph_cases().items()):
        c.execute(f"CREATE TABLE t_{name}(s TEXT, d TEXT, w REAL)")
        c.executemany(f"INSERT INTO t_{name} VALUES (?, ?, ?)", rows)
        out["paths"][name] = []
        for q in tm.path_queries()[name]:
            got = c.execute(f"SELECT node, distance, path_order FROM graph_shortest_path('t_{name}', 's', 'd', ?, ?, 'w') "
                            f"ORDER BY path_order", q).fetchall()
            assert [r[2] for r in got] == list(range(len(got)))
            out["paths"][name].append([[r[0], r[1].hex()] for r in got])
            n_ambiguous += ambiguous(rows, q[0], [r[0] for r in got])
    out["schema"] = [[r[1], r[2], r[6]] for r in c.execute("SELECT * FROM pragma_table_xinfo('graph_shortest_path')")]
    c.close()
    # without a path that could have gone another way the rows cannot tell a wrong tie-break from a right one
    assert n_ambiguous > 0, "no recorded path is ambiguous"
    out["ambiguous"] = n_ambiguous
    c = ref_conn()
    ts.fill_tables(c)
    for name, sql in sorted({**ts.HOST_STATEMENTS, **ts.DEVICE_STATEMENTS}.items()):
        out["sql"][name] = ts.answer(c, sql)
        print(name, "→", out["sql"][name].get("error") or f"{len(out['sql'][name]['rows'])} rows")
    c.close()
    every = [p for v in out["paths"].values() for p in v]
    with gzip.GzipFile(OUT, "wb", 9, mtime=0) as f:
        f.write(json.dumps(out, separators=(",", ":")).encode())
    print(os.path.relpath(OUT, ROOT), os.path.getsize(OUT), "bytes;", len(every), "paths,", sum(len(p) > 0 for p in every), "found,",
          n_ambiguous, "ambiguous,", len(out["sql"]), "statements")


if __name__ == "__main__":
    main()
