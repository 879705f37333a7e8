"""Writes tests/golden/tvf_statements.json.gz: what the REFERENCE's ten graph table-valued functions answer (oracle/_ref/muninn.so
through sqlite3) for the statements of tests/test_tvf_statements.py: rows, or the error's text.  Runs only where the compiled
reference exists; the test reads the file.  Recorded answers only.

    python scripts/gen_tvf_statements_golden.py
"""
import gzip
import json
import os
import sqlite3
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import test_tvf_statements as ts  # noqa: E402
from oracle import orc_graph as og  # noqa: E402


def main():
    assert og.have_ref_graph(), "oracle/_ref/muninn.so is not built"
    c = sqlite3.connect(":memory:")
    c.enable_load_extension(True)
    c.load_extension(og.REF_EXT_SO[:-3])
    ts.fill_tables(c)
    out = {}
    for key, statements in (("host", ts.HOST_STATEMENTS), ("schema", ts.SCHEMAS), ("plan", ts.PLANS), ("device", ts.DEVICE_STATEMENTS)):
        out[key] = {}
        for name, sql in sorted(statements.items()):
            out[key][name] = got = ts.answer(c, sql)
            print(key, name, "→", got.get("error") or got["rows"][:2])
    c.close()
    # the statements must be able to tell one rule, one default and one function from another
    assert all("rows" in a and len(a["rows"]) >= 5 for a in out["device"].values()), "a device statement has no answer to compare"
    for f, extra in ts.DEVICE_EXTRA.items():
        assert not extra or out["device"][f"{f}/all_hidden"] != out["device"][f"{f}/required"], f"{f}: the hidden columns change nothing"
    assert len({json.dumps(a) for a in out["schema"].values()}) == len(ts.ALL_TEN), "two functions declare one schema"
    assert len({a["error"] for a in out["host"].values() if "error" in a}) >= 8, "fewer than eight different error strings"
    with gzip.GzipFile(ts.GOLDEN, "wb", 9, mtime=0) as f:
        f.write(json.dumps(out, separators=(",", ":")).encode())
    print(os.path.relpath(ts.GOLDEN, ROOT), os.path.getsize(ts.GOLDEN), "bytes;", sum(len(v) for v in out.values()), "statements")


if __name__ == "__main__":
    main()
