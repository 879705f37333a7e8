"""Writes tests/golden/er.json.gz: what the REFERENCE answers for the entity-resolution tests.

The reference compiles muninn_extract_er only together with llama.cpp, although the function uses no model, so
oracle/_ref/muninn.so (built with -DMUNINN_NO_LLAMA) does not contain it.  This script compiles the reference's llama_er.c and
string_sim.c where they lie, with a registering shim, into a temporary directory (nothing is written under oracle/), loads the
result next to oracle/_ref/muninn.so and records

  jw       the f64 bits of jaro_winkler for tests/er_model.py's fixed pair list
  grid     the inputs (entities, vectors) and, per case, the arguments and the JSON text muninn_extract_er returned
  sqlite_slots   the slot of sqlite3_result_subtype in the reference's vendored sqlite3ext.h (ext/mn_er_sql.c hard-codes it)

Runs only where the reference's sources and the compiled reference exist; the tests read the file.

    python scripts/gen_er_golden.py
"""
import ctypes as C
import gzip
import json
import os
import sqlite3
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import er_model as em  # noqa: E402
from oracle import orc_graph as og  # noqa: E402

REF = os.environ.get("REF", "/root/reference")
OUT = os.path.join(ROOT, "tests", "golden", "er.json.gz")
DIM = 16

SHIM = """
#include "sqlite3ext.h"
SQLITE_EXTENSION_INIT1
#include "llama_er.h"
int sqlite3_erref_init(sqlite3 *db, char **err, const sqlite3_api_routines *api) {
    (void)err;
    SQLITE_EXTENSION_INIT2(api);
    return llama_er_register_functions(db);
}
"""


def build_ref(tmp):
    shim = os.path.join(tmp, "er_shim.c")
    with open(shim, "w") as f:
        f.write(SHIM)
    so = os.path.join(tmp, "erref.so")
    src = os.path.join(REF, "src")
    subprocess.run(["gcc", "-O2", "-std=c11", "-fPIC", "-D_POSIX_C_SOURCE=200809L", "-shared", "-I" + src, "-o", so,
                    os.path.join(src, "llama_er.c"), os.path.join(src, "string_sim.c"), shim, "-lm"], check=True)
    return so


def unit(angle_deg, ax0, ax1):
    v = np.zeros(DIM, np.float32)
    v[ax0] = np.cos(np.radians(angle_deg))
    v[ax1] = np.sin(np.radians(angle_deg))
    return v


def dataset():
    """(rows, vectors): rows = [(rowid, entity_id, name, source)], vectors = {rowid: f32[DIM]} (a row without one has no vector).
    Overlapping groups, a single-edge bridge between two pairs, pairs that only one guard mode or one jw_weight keeps."""
    rng = np.random.default_rng(7)
    rows, vec = [], {}

    def add(eid, name, source, v):
        rowid = 3 * len(rows) + 2  # not contiguous, not starting at 1
        rows.append((rowid, eid, name, source))
        if v is not None:
            vec[rowid] = (np.asarray(v, np.float32) + rng.normal(0, 0.004, DIM).astype(np.float32)).astype(np.float32)

    # one tight group of five: byte-equal names, names equal after lowering, edits; mixed sources
    for i, (nm, src) in enumerate([("Jonathan Smith", "a"), ("Jonathan Smith", "b"), ("JONATHAN SMITH", "a"), ("Jonathon Smith", "b"),
                                   ("Jonathan Smyth", "")]):
        add(f"p{i}", nm, src, unit(4 * i, 0, 1))
    # two pairs on one circle, 40 degrees between their inner ends: the only edge between them is a bridge
    for eid, nm, src, ang in [("acme1", "Acme Corp", "x", 0), ("acme2", "Acme Corp.", "x", 20), ("acme3", "Acme Corporation", "y", 60),
                              ("acme4", "ACME Corporation", "y", 80)]:
        add(eid, nm, src, unit(ang, 2, 3))
    # close vectors, unlike names: kept by the cosine term alone
    add("ibm1", "IBM", "s", unit(0, 4, 5))
    add("ibm2", "International Business Machines", "s", unit(8, 4, 5))
    # like names, vectors near the threshold: kept by the name term alone once borderline_delta lifts the bar
    add("geo1", "Globex Industries", "m", unit(0, 6, 7))
    add("geo2", "Globex Industry", "n", unit(43, 6, 7))
    # a path of three (its ends 50 degrees apart: no edge) with different types: Leiden keeps it whole, diff_type and the bridge cut
    # take it apart
    add("ch1", "Initech", "person", unit(0, 8, 9))
    add("ch2", "Initech LLC", "place", unit(25, 8, 9))
    add("ch3", "Initech L.L.C.", "person", unit(50, 8, 9))
    # an id json_escape has work with; a row without a vector; a row whose vector is deleted in the second state
    add('q"uo\\te\tid', "Hooli", "", unit(0, 10, 11))
    add("novec", "Hooli", "", None)
    add("gone", "Hooli", "z", unit(5, 10, 11))
    # fillers: random directions, far from everything
    for i in range(24):
        v = rng.normal(0, 1, DIM)
        add(f"f{i}", "".join(chr(97 + c) for c in rng.integers(0, 26, rng.integers(5, 12))), "abc"[i % 3], v / np.linalg.norm(v))
    return rows, vec


def open_db(erso, rows, vec, deleted=()):
    c = sqlite3.connect(":memory:")
    c.enable_load_extension(True)
    c.load_extension(og.REF_EXT_SO[:-3])
    c.load_extension(erso[:-3])  # erref.so -> sqlite3_erref_init
    c.execute(f"CREATE VIRTUAL TABLE vec USING hnsw_index(dimensions={DIM}, metric='cosine')")
    c.execute("CREATE TABLE entities(entity_id TEXT, name TEXT, source TEXT)")
    for rowid, eid, name, source in rows:
        c.execute("INSERT INTO entities(rowid, entity_id, name, source) VALUES (?, ?, ?, ?)", (rowid, eid, name, source))
        if rowid in vec:
            c.execute("INSERT INTO vec(rowid, vector) VALUES (?, ?)", (rowid, vec[rowid].tobytes()))
    for rowid in deleted:
        c.execute("DELETE FROM vec WHERE rowid = ?", (rowid,))
    c.commit()
    return c


def call(c, args):
    sql = "SELECT muninn_extract_er('vec', 'name', " + ", ".join("?" for _ in args) + ")"
    return c.execute(sql, args).fetchone()[0]


def knn(c, rows, k):
    """the lists the reference's loop sees (src/llama_er.c:237-284), for the model"""
    n = len(rows)
    ids = np.full((n, k + 1), -1, np.int64)
    ds = np.zeros((n, k + 1), np.float32)
    cnt = np.zeros(n, np.int32)
    for i, (rowid, *_rest) in enumerate(rows):
        r = c.execute("SELECT vector FROM vec WHERE rowid = ?", (rowid,)).fetchone()
        if r is None:
            continue
        got = c.execute(f"SELECT rowid, distance FROM vec WHERE vector MATCH ? AND k = {k + 1}", (r[0],)).fetchall()
        cnt[i] = len(got)
        for p, (nid, d) in enumerate(got):
            ids[i, p] = nid
            ds[i, p] = d
    return ids, ds, cnt


def branches_of(c, rows, args):
    k, thr, w, delta = args[:4]
    guard = args[6] if len(args) > 6 else None
    ids, ds, cnt = knn(c, rows, k)
    cands = em.candidates([r[0] for r in rows], ids, ds, cnt, thr)
    hit = {}
    em.cascade(cands, [r[2].encode() for r in rows], [r[3].encode() for r in rows], guard, w, 1.0 - thr + delta, hit)
    return hit


def clusters_of(js):
    by = {}
    for key, cl in json.loads(js)["clusters"].items():
        by.setdefault(cl, []).append(key)
    return by


def main():
    assert og.have_ref_graph(), "oracle/_ref/muninn.so is not built"
    with tempfile.TemporaryDirectory() as tmp:
        erso = build_ref(tmp)
        L = C.CDLL(erso)
        L.jaro_winkler.restype = C.c_double
        L.jaro_winkler.argtypes = [C.c_char_p, C.c_char_p]
        jw = []
        for a, b in em.fixed_pairs():
            assert 0 not in a and 0 not in b
            got = L.jaro_winkler(a, b)
            assert em.bits(got) == em.bits(em.jaro_winkler(a, b)), (a, b)
            jw.append([a.hex(), b.hex(), em.bits(got)])
        rng = np.random.default_rng(99)
        for _ in range(20000):  # the model against the compiled reference, beyond the recorded list
            al = [b"ab", b"abcd", bytes(range(1, 256))][rng.integers(0, 3)]
            a, b = em.rand_name(rng, int(rng.integers(0, 90)), al), em.rand_name(rng, int(rng.integers(0, 90)), al)
            assert em.bits(L.jaro_winkler(a, b)) == em.bits(em.jaro_winkler(a, b)), (a, b)

        rows, vec = dataset()
        gone = [r[0] for r in rows if r[1] == "gone"]
        N = None
        base = [4, 0.3, 0.5, 0.0]
        states = {"main": (), "after_delete": tuple(gone)}
        # the bridge's betweenness is read from the reference so that the threshold sits between it and the next edge's
        c = open_db(erso, rows, vec)
        cases = {
            "base": base,
            "jw0": [4, 0.3, 0.0, 0.05],
            "jw05": [4, 0.3, 0.5, 0.05],
            "jw1": [4, 0.3, 1.0, 0.05],
            "delta": [4, 0.3, 0.5, 0.1],
            "k1": [1, 0.3, 0.5, 0.0],
            "k10": [10, 0.3, 0.5, 0.0],
            "tight": [4, 0.05, 0.5, 0.0],
            "wide": [6, 1.2, 0.2, 0.0],
            "chat_ignored": base + ["some-model"],
            "eb_null": base + [N, N],
            "unguarded": base + [N, N, ""],
            "unknown_guard": base + [N, N, "bogus"],
            "same_source": base + [N, N, "same_source"],
            "diff_type": base + [N, N, "diff_type"],
        }
        ebs = sorted({round(r[0], 9) for r in edge_betweenness(c, rows, base)}, reverse=True)
        print("edge betweenness values:", ebs[:6])
        assert len(ebs) >= 2
        cases["eb_cut_top"] = base + [N, (ebs[0] + ebs[1]) / 2]  # only the most central edge goes
        cases["eb_cut"] = base + [N, (ebs[-1] + ebs[-2]) / 2]    # every edge that is not inside a clique goes
        cases["eb_cut_all"] = base + [N, 0.0]
        cases["eb_none"] = base + [N, ebs[0] + 1.0]
        grid = {}
        hits = {b: 0 for b in em.BRANCHES}
        for state, deleted in states.items():
            cs = open_db(erso, rows, vec, deleted)
            grid[state] = {}
            for name, args in cases.items():
                want, n_bridges = compose(cs, rows, args)
                if n_bridges == 0:
                    js = call(cs, args)
                    assert js == want, (state, name, js, want)  # the composition below is the function, where the function runs
                else:
                    js = want
                json.loads(js)
                grid[state][name] = {"args": args, "json": js, "composed": n_bridges > 0}
                for b, v in branches_of(cs, rows, args).items():
                    hits[b] += v
            cs.close()
        c.close()

        # the recorded grid is not vacuous (tests/test_er_model.py asserts the same on the file)
        g = grid["main"]
        sizes = sorted(len(v) for v in clusters_of(g["base"]["json"]).values())
        assert sizes[-1] >= 3 and sizes[0] == 1, sizes
        assert g["same_source"]["json"] != g["unguarded"]["json"] != g["diff_type"]["json"] != g["same_source"]["json"]
        assert g["eb_cut"]["json"] != g["eb_null"]["json"], "no bridge was cut"
        assert len({g["jw0"]["json"], g["jw05"]["json"], g["jw1"]["json"]}) > 1
        assert all(hits[b] > 0 for b in em.BRANCHES), hits
        assert grid["after_delete"]["base"]["json"] != g["base"]["json"]
        print("clusters (base):", sorted(clusters_of(g["base"]["json"]).values(), key=len, reverse=True)[:6])
        print("clusters (eb_cut):", sorted(clusters_of(g["eb_cut"]["json"]).values(), key=len, reverse=True)[:6])
        print("branches:", hits)

        from oracle import sqlite_abi
        slots, _ = sqlite_abi.measure(os.path.join(REF, "src", "sqlite3ext.h"), tmp, ["result_subtype"])
        out = {"jw": jw, "dim": DIM, "branches": hits, "sqlite_slots": slots,
               "entities": [[r[0], r[1], r[2], r[3], vec[r[0]].tobytes().hex() if r[0] in vec else None] for r in rows],
               "states": {s: list(d) for s, d in states.items()}, "grid": grid}
        with gzip.GzipFile(OUT, "wb", 9, mtime=0) as f:
            f.write(json.dumps(out, separators=(",", ":")).encode())
        print(OUT, os.path.getsize(OUT), "bytes,", len(jw), "pairs,", sum(len(v) for v in grid.values()), "cases")


def json_key(s):
    """src/llama_er.c:68-110"""
    out = []
    for ch in s.encode():
        if ch == 0x22:
            out.append('\\"')
        elif ch == 0x5C:
            out.append("\\\\")
        elif ch == 0x0A:
            out.append("\\n")
        elif ch == 0x0D:
            out.append("\\r")
        elif ch == 0x09:
            out.append("\\t")
        elif ch < 0x20:
            out.append("\\u%04x" % ch)
        else:
            out.append(bytes([ch]).decode("latin-1"))
    return '"' + "".join(out).encode("latin-1").decode("utf-8") + '"'


def compose(c, rows, args):
    """(JSON, bridges cut): muninn_extract_er put together from its parts — the reference's own searches, graph_leiden and
    graph_edge_betweenness through SQL, the model for the lines between (src/llama_er.c:237-332) and the glue of :334-574
    restated here.  Where the reference's function runs, main() asserts that it returns this very text.  It does not run when an
    edge exceeds the betweenness threshold: its two bridge arrays share one capacity counter (:465-466), the second is never
    allocated, and the first bridge is written through a null pointer.  Those cases are recorded from this composition and
    marked "composed"."""
    k, thr, w, delta = args[:4]
    eb = args[5] if len(args) > 5 and args[5] is not None else -1.0
    guard = args[6] if len(args) > 6 else None
    ids, ds, cnt = knn(c, rows, k)
    cands = em.candidates([r[0] for r in rows], ids, ds, cnt, thr)
    edges = em.cascade(cands, [r[2].encode() for r in rows], [r[3].encode() for r in rows], guard, w, 1.0 - thr + delta)
    eid = [r[1] for r in rows]
    c.execute("DROP TABLE IF EXISTS temp._er_edges")
    c.execute("CREATE TEMP TABLE _er_edges(src TEXT, dst TEXT, weight REAL)")
    for i, j, s in edges:
        c.execute("INSERT INTO temp._er_edges VALUES (?, ?, ?)", (eid[i], eid[j], s))
        c.execute("INSERT INTO temp._er_edges VALUES (?, ?, ?)", (eid[j], eid[i], s))

    def leiden(run):
        cluster, remap = [-1] * len(rows), {}
        if run:
            for node, com in c.execute("SELECT node, community_id FROM graph_leiden WHERE edge_table = '_er_edges' AND src_col = 'src'"
                                       " AND dst_col = 'dst' AND weight_col = 'weight'").fetchall():
                if node in eid:
                    cluster[eid.index(node)] = remap.setdefault(com, len(remap))
        nxt = len(remap)
        for i in range(len(rows)):
            if cluster[i] < 0:
                cluster[i] = nxt
                nxt += 1
        return cluster

    cluster = leiden(len(edges) > 0)
    n_bridges = 0
    if eb >= 0 and edges:
        bridges = [(s, d) for s, d, bc in c.execute("SELECT src, dst, centrality FROM graph_edge_betweenness WHERE edge_table ="
                                                    " '_er_edges' AND src_col = 'src' AND dst_col = 'dst' AND direction = 'both'")
                   if bc > eb]
        n_bridges = len(bridges)
        for s, d in bridges:
            c.execute("DELETE FROM temp._er_edges WHERE (src = ? AND dst = ?) OR (src = ? AND dst = ?)", (s, d, d, s))
        if bridges:
            cluster = leiden(True)
    c.execute("DROP TABLE IF EXISTS temp._er_edges")
    return '{"clusters":{' + ",".join(f"{json_key(eid[i])}:{cluster[i]}" for i in range(len(rows))) + "}}", n_bridges


def edge_betweenness(c, rows, args):
    """centrality of every edge of the base case's match graph, from the reference's own graph_edge_betweenness over the edges the
    model derives (the function under record drops its temp table before it returns)"""
    k, thr, w, delta = args[:4]
    ids, ds, cnt = knn(c, rows, k)
    cands = em.candidates([r[0] for r in rows], ids, ds, cnt, thr)
    edges = em.cascade(cands, [r[2].encode() for r in rows], [r[3].encode() for r in rows], None, w, 1.0 - thr + delta)
    c.execute("CREATE TEMP TABLE _probe(src TEXT, dst TEXT, weight REAL)")
    for i, j, s in edges:
        c.execute("INSERT INTO _probe VALUES (?, ?, ?)", (rows[i][1], rows[j][1], s))
        c.execute("INSERT INTO _probe VALUES (?, ?, ?)", (rows[j][1], rows[i][1], s))
    out = c.execute("SELECT centrality, src, dst FROM graph_edge_betweenness WHERE edge_table = '_probe' AND src_col = 'src'"
                    " AND dst_col = 'dst' AND direction = 'both'").fetchall()
    c.execute("DROP TABLE _probe")
    return out


if __name__ == "__main__":
    main()
