"""Writes tests/golden/centrality.json.gz and tests/golden/centrality_large.npz: what the REFERENCE's graph_closeness and
graph_degree return (oracle/_ref/muninn.so through sqlite3, as oracle.orc_graph.ref_betweenness_sql loads it) for the cases
of tests/test_centrality.py.  Runs only where the compiled reference exists; the tests read the two files.

    python scripts/gen_centrality_golden.py
"""
import gzip
import json
import os
import shutil
import sqlite3
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import test_centrality as tc  # noqa: E402
from oracle import orc_graph as og  # noqa: E402

G = os.path.join(ROOT, "tests", "golden")


def ref_conn(path=":memory:"):
    c = sqlite3.connect(path)
    c.enable_load_extension(True)
    c.load_extension(og.REF_EXT_SO[:-3])
    return c


def record(c, where):
    nodes, cc, dnodes, deg = tc.run_tvfs(c, where)
    return {"nodes": nodes, "cc_bits": cc, "deg_nodes": dnodes, "deg_bits": deg}


def main():
    assert og.have_ref_graph(), "oracle/_ref/muninn.so is not built"
    c = ref_conn()
    out = {"small": {}, "edge": {}, "errors": {}}
    for name, (rows, weighted, direction, normalized) in sorted(tc.small_cases().items()):
        tc.fill_edge_table(c, rows)
        out["small"][name] = record(c, tc.where_of(weighted, direction, normalized))
    tc.fill_edge_case_table(c)
    for key, extra in tc.EDGE_QUERIES.items():
        out["edge"][key] = record(c, "edge_table='ec' AND src_col='s' AND dst_col='d' AND " + extra)
    for tvf in ("graph_closeness", "graph_degree"):
        out["errors"][tvf] = {}
        for key, where in tc.ERROR_QUERIES.items():
            try:
                c.execute(f"SELECT * FROM {tvf} WHERE {where}").fetchall()
                raise AssertionError((tvf, key, "no error"))
            except sqlite3.OperationalError as e:
                out["errors"][tvf][key] = str(e)
    large = {}
    for name, (rows, weighted, direction, normalized) in sorted(tc.large_cases().items()):
        tc.fill_edge_table(c, rows)
        r = record(c, tc.where_of(weighted, direction, normalized))
        assert r["nodes"] == r["deg_nodes"]
        large[name + "_nodes"] = np.array(r["nodes"])
        large[name + "_cc"] = np.asarray(r["cc_bits"], np.int64)
        large[name + "_deg"] = np.asarray(r["deg_bits"], np.int64)
    c.close()
    want_nodes = np.load(os.path.join(G, "adjacency.npz"))
    with tempfile.TemporaryDirectory() as tmp:
        for state in ("fresh", "stale"):
            db = os.path.join(tmp, f"adjacency_{state}.db")
            with gzip.open(os.path.join(G, f"adjacency_{state}.db.gz"), "rb") as fi, open(db, "wb") as fo:
                shutil.copyfileobj(fi, fo)
            c = ref_conn(db)
            r = record(c, "edge_table='g' AND src_col='src' AND dst_col='dst'")
            c.close()
            assert r["nodes"] == r["deg_nodes"] == want_nodes[f"{state}_nodes"].tolist()
            large[f"adjacency_{state}_cc"] = np.asarray(r["cc_bits"], np.int64)
            # four more arrays of this size would outweigh every other golden: their SHA-256 (little-endian bits) instead
            large[f"adjacency_{state}_deg_sha256"] = np.array([tc.sha_of(np.asarray(col, np.int64).view(np.float64))
                                                               for col in r["deg_bits"]])
            print(state, len(r["nodes"]), "nodes,", sum(b == 0 for b in r["cc_bits"]), "with closeness 0")
    with gzip.GzipFile(os.path.join(G, "centrality.json.gz"), "wb", 9, mtime=0) as f:
        f.write(json.dumps(out, separators=(",", ":")).encode())
    np.savez_compressed(os.path.join(G, "centrality_large.npz"), **large)
    for f in ("centrality.json.gz", "centrality_large.npz"):
        print(f, os.path.getsize(os.path.join(G, f)), "bytes")
    first = out["edge"]["weight"]
    print("edge/weight:", first["nodes"], np.asarray(first["cc_bits"], np.int64).view(np.float64).tolist())
    print("edge/window:", out["edge"]["window"]["nodes"])


if __name__ == "__main__":
    main()
