"""Writes tests/golden/select.json.gz: what the REFERENCE's graph_select returns (oracle/_ref/muninn.so through sqlite3) for the
grid of tests/test_select_model.py and the statements of tests/test_select_sql.py.  Runs only where the compiled reference
exists; the tests read the file.  Recorded rows and error strings only.

    python scripts/gen_select_golden.py
"""
import gzip
import json
import os
import sqlite3
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import test_select_model as tm  # noqa: E402
import test_select_sql as ts  # noqa: E402
from oracle import orc_graph as og  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "select.json.gz")


def ref_conn():
    c = sqlite3.connect(":memory:")
    c.enable_load_extension(True)
    c.load_extension(og.REF_EXT_SO[:-3])
    return c


def main():
    assert og.have_ref_graph(), "oracle/_ref/muninn.so is not built"
    out = {"select": {}, "sql": {}}
    c = ref_conn()
    ts.fill_case_tables(c)
    for name, exprs in sorted(tm.selectors().items()):
        out["select"][name] = [ts.case_answer(c, name, expr) for expr in exprs]
    c.close()
    c = ref_conn()
    ts.fill_tables(c)
    for name, sql in sorted({**ts.HOST_STATEMENTS, **ts.DEVICE_STATEMENTS}.items()):
        out["sql"][name] = ts.answer(c, sql)
        print(name, "→", out["sql"][name].get("error") or f"{len(out['sql'][name]['rows'])} rows")
    c.close()
    # the grid must be able to tell a wrong evaluator from a right one
    z = out["select"]
    at = lambda name, expr: z[name][tm.selectors()[name].index(expr)]
    rows = lambda a: {r[1]: r[2] for r in a["rows"]}
    apart = dict(rows(at("cyclic", "a+")))
    apart.update({k: min(v, apart.get(k, v)) for k, v in rows(at("cyclic", "+a")).items()})
    assert rows(at("cyclic", "+a+")) != apart, "no +x+ differs from its ancestors and descendants computed separately"
    assert set(rows(at("cyclic", "1+a+3"))) != set(rows(at("cyclic", "1+a"))) | set(rows(at("cyclic", "a+3"))), \
        "no limited N+x+M differs as a set from N+x and x+M computed separately"
    assert set(rows(at("words", "1+c b"))) > set(rows(at("words", "1+c"))) | {"b"}, "no limit under a union is ignored"
    assert set(rows(at("words", "a+0 c"))) == {"a", "c"} and len(rows(at("words", "a+"))) > 1, "no limit of 0 under a union is honoured"
    assert any(max(rows(a).values(), default=0) > 0 for e, a in zip(tm.selectors()["dag"], z["dag"]) if e.startswith("@")), \
        "no @x gives a depth above 0"
    errors = {a["error"] for case in z.values() for a in case if "error" in a} | \
             {a["error"] for a in out["sql"].values() if "error" in a}
    for want in ("graph_select: empty selector expression", "graph_select: expected node name at position 0",
                 "graph_select: unexpected character '$' at position 1", "graph_select: node 'nosuch' not found",
                 "graph_select: requires edge_table, src_col, dst_col, selector", "graph_select: NULL parameter not allowed",
                 "graph_select: invalid table/column identifier", "graph_select: failed to prepare: no such table: nope"):
        assert want in errors, want
    assert any(len(e.encode()) == 255 for e in errors), "no message is cut at 255 bytes"
    with gzip.GzipFile(OUT, "wb", 9, mtime=0) as f:
        f.write(json.dumps(out, separators=(",", ":")).encode())
    print(os.path.relpath(OUT, ROOT), os.path.getsize(OUT), "bytes;", sum(len(v) for v in z.values()), "selectors,",
          len(out["sql"]), "statements,", len(errors), "distinct error strings")


if __name__ == "__main__":
    main()
