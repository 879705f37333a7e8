"""Writes tests/golden/adjacency_vtab.json.gz: the sessions of tests/adjacency_sessions.py as the REFERENCE's graph_adjacency
answers them (oracle/_ref/muninn.so through sqlite3), statement by statement, with the shadow tables, triggers and declared
columns at every checkpoint.  Runs only where the compiled reference exists; the tests read the file.  Recorded results only.

    python scripts/gen_adjacency_golden.py
"""
import gzip
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import adjacency_sessions as sess  # noqa: E402
from oracle import orc_graph as og  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "adjacency_vtab.json.gz")


def main():
    assert og.have_ref_graph(), "oracle/_ref/muninn.so is not built"
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        for name in sess.SESSIONS:
            out[name] = sess.run(name, lambda c: c.load_extension(og.REF_EXT_SO[:-3]), tmp)
            errs = sum(isinstance(line, list) and isinstance(line[1], dict) for line in out[name])
            print(f"{name}: {len(out[name])} lines, {errs} errors")
    # the sessions must reach what they are there for
    cfg = lambda d: dict((k, v) for k, v in d["_config"])  # noqa: E731
    dumps = {name: [line for line in t if isinstance(line, dict)] for name, t in out.items()}
    for name, merged_edges in (("thresholds_small", "20"), ("thresholds_larger", "251")):
        first, second = dumps[name]
        assert cfg(first)["edge_count"] == merged_edges, (name, cfg(first))  # by log rows: a merge ran
        ids1, ids2 = [r[1] for r in first["_nodes"]], [r[1] for r in second["_nodes"]]
        assert ids1[-1].startswith("x") and ids2[:len(ids1)] != ids1, name  # appended by the merge, renumbered by the full rebuild
    assert len(dumps["nodes_4096_then_one_more"][0]["_csr_fwd"]) == 1 and len(dumps["nodes_4096_then_one_more"][1]["_csr_fwd"]) == 2
    assert len(dumps["nodes_4097"][0]["_csr_fwd"]) == 2
    assert any("NEW.NULL" in str(line) for line in out["unweighted_integers"])
    with gzip.GzipFile(OUT, "wb", 9, mtime=0) as f:
        f.write(json.dumps(out, separators=(",", ":")).encode())
    print(os.path.relpath(OUT, ROOT), os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
