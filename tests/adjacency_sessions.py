"""SQL sessions on the graph_adjacency virtual table, written once and run twice: by scripts/gen_adjacency_golden.py under
the REFERENCE's extension, which records them into tests/golden/adjacency_vtab.json.gz, and by tests/test_adjacency_vtab.py
under this project's.  A session is a function of a Recorder; the transcript is a list of JSON values: per statement its rows
or its error text, per checkpoint the six shadow tables, the trigger rows of sqlite_master and pragma_table_xinfo.  Floats are
recorded as hex (every bit counts), blobs as hex up to 64 bytes and as sha256 + length beyond."""
import hashlib
import os
import sqlite3

import numpy as np

SHADOWS = ("_config", "_nodes", "_degree", "_csr_fwd", "_csr_rev", "_delta")
TVFS = ("graph_degree", "graph_closeness", "graph_node_betweenness", "graph_edge_betweenness")


def enc(v):
    if isinstance(v, float):
        return ["f", v.hex()]
    if isinstance(v, (bytes, memoryview)):
        b = bytes(v)
        return ["b", b.hex()] if len(b) <= 64 else ["sha256", hashlib.sha256(b).hexdigest(), len(b)]
    return v


class Recorder:
    def __init__(self, load, path=":memory:"):
        self.load, self.path, self.out = load, path, []
        self.c = None
        self.open()

    def open(self):
        self.c = sqlite3.connect(self.path, isolation_level=None)  # autocommit: BEGIN / ROLLBACK are the session's own
        self.c.enable_load_extension(True)
        self.load(self.c)

    def reopen(self):
        self.c.close()
        self.open()
        self.out.append("reopened")

    def close(self):
        self.c.close()

    def x(self, sql, params=()):
        try:
            rows = self.c.execute(sql, params).fetchall()
            self.out.append([sql, [[enc(v) for v in r] for r in rows]])
        except sqlite3.Error as e:
            self.out.append([sql, {"error": str(e)}])

    def many(self, sql, rows):
        rows = list(rows)
        try:
            self.c.execute("BEGIN")
            self.c.executemany(sql, rows)
            self.c.execute("COMMIT")
            self.out.append([sql, len(rows)])
        except sqlite3.Error as e:
            self.out.append([sql, {"error": str(e)}])
            if self.c.in_transaction:
                self.c.execute("ROLLBACK")

    def dump(self, t="g"):
        d = {}
        for s in SHADOWS:
            try:
                d[s] = [[enc(v) for v in r] for r in self.c.execute(f'SELECT * FROM "{t}{s}" ORDER BY 1')]
            except sqlite3.Error as e:
                d[s] = {"error": str(e)}
        d["triggers"] = [list(r) for r in self.c.execute("SELECT name, tbl_name, sql FROM sqlite_master WHERE type='trigger' ORDER BY name")]
        try:
            d["xinfo"] = [list(r) for r in self.c.execute(f"SELECT * FROM pragma_table_xinfo('{t}')")]
        except sqlite3.Error as e:
            d["xinfo"] = {"error": str(e)}
        self.out.append(d)

    def tvfs(self, t="g", s="s", d="d"):
        """the graph functions over the adjacency table (they are given the table's own column names, as the reference's tests do)"""
        where = f"edge_table='{t}' AND src_col='{s}' AND dst_col='{d}'"
        self.x(f"SELECT node, community_id, modularity FROM graph_leiden WHERE {where}")
        for f in TVFS:
            self.x(f"SELECT * FROM {f} WHERE {where}")


WEIGHTED = "CREATE VIRTUAL TABLE g USING graph_adjacency(edge_table='e', src_col='s', dst_col='d', weight_col='w')"
SMALL = [("a", "b", 1.5), ("b", "c", 0.25), ("a", "b", 2.0), ("c", "c", 1.0), (None, "a", 1.0), ("a", None, 1.0), ("c", "a", 0.5),
         ("d", "a", 4.0), ("b", "d", 1.0), ("e", "f", 3.0), ("a", "b", 0.125), ("f", "e", 1.0)]


def weighted_small(r):
    """NULL ends, duplicates, a self-loop; fresh and stale graph functions; refresh by SELECT, by both commands; deletes of
    present and absent edges; UPDATE; commands and their errors"""
    r.x("CREATE TABLE e(s TEXT, d TEXT, w REAL)")
    r.many("INSERT INTO e VALUES (?, ?, ?)", SMALL)
    r.x(WEIGHTED)
    r.dump()
    r.x("SELECT * FROM g")
    r.x("SELECT node, node_idx, in_degree, out_degree, weighted_in_degree, weighted_out_degree, g FROM g WHERE node = 'a'")
    r.x("SELECT rowid, node FROM g WHERE node = 'nope'")
    r.x("SELECT count(*) FROM g WHERE out_degree > 1")
    r.tvfs()
    r.x("INSERT INTO e VALUES ('a', 'z', 9.0), ('z', 'b', 0.5), ('c', 'c', 2.0)")
    r.x("SELECT count(*) FROM g_delta")
    r.tvfs()  # stale: answered from the edge table, the log stays
    r.x("SELECT count(*) FROM g_delta")
    r.x("SELECT * FROM g")  # refresh by SELECT: 3 <= 10 → incremental
    r.dump()
    r.x("DELETE FROM e WHERE s = 'nobody'")
    r.x("DELETE FROM e WHERE s = 'a' AND d = 'b' AND w = 2.0")
    r.x("UPDATE e SET w = 7.0, d = 'q' WHERE s = 'e'")
    r.x("INSERT INTO g_delta(src, dst, weight, op) VALUES ('zz', 'a', 1.0, 2), ('a', 'nowhere', 1.0, 2), (NULL, 'a', 1.0, 1)")
    r.x("INSERT INTO g(g) VALUES ('incremental_rebuild')")
    r.dump()
    r.x("SELECT * FROM g")
    r.tvfs()
    r.x("INSERT INTO g(g) VALUES ('incremental_rebuild')")  # empty log: nothing happens
    r.x("INSERT INTO g(g) VALUES ('stats')")
    r.x("INSERT INTO g(g) VALUES ('rebuild')")
    r.dump()
    r.x("INSERT INTO g(g) VALUES ('nope')")
    r.x("INSERT INTO g(g) VALUES (NULL)")
    r.x("INSERT INTO g(node) VALUES ('x')")
    r.x("INSERT INTO g(g) VALUES (42)")
    r.x("DELETE FROM g WHERE node = 'a'")
    r.x("UPDATE g SET node = 'x' WHERE node = 'a'")
    r.x("DROP TABLE g")
    r.dump()
    r.x("INSERT INTO e VALUES ('after', 'drop', 1.0)")


def unweighted_integers(r):
    """no weight column: the table builds and reads, every later change of the edge table fails on the trigger text; integer ids"""
    r.x("CREATE TABLE e(s INTEGER, d INTEGER)")
    r.many("INSERT INTO e VALUES (?, ?)", [(1, 2), (2, 3), (3, 1), (10, 2), (2, 2), (1, 2), (7, None), (3, 10)])
    r.x("CREATE VIRTUAL TABLE g USING graph_adjacency(edge_table=e, src_col=\"s\", dst_col='d')")
    r.dump()
    r.x("SELECT * FROM g")
    r.x("SELECT * FROM g WHERE node = 10")
    r.x("SELECT * FROM g WHERE node = '10'")
    r.tvfs()
    r.x("INSERT INTO e VALUES (4, 5)")
    r.x("DELETE FROM e WHERE s = 1")
    r.x("UPDATE e SET d = 9 WHERE s = 10")
    r.x("SELECT count(*) FROM e")
    r.x("INSERT INTO g(g) VALUES ('rebuild')")
    r.x("INSERT INTO g(g) VALUES ('incremental_rebuild')")
    r.dump()


def _ring(n, k, seed):
    rng = np.random.default_rng(seed)
    return [(f"n{i}", f"n{(i + 1 + int(j)) % n}", float(rng.integers(1, 9)) * 0.25) for i in range(n) for j in rng.integers(0, n - 1, k)]


def _changes(r, rows, n_del, n_ins, tag):
    """n_del single-row deletes and n_ins inserts (every third one names a new node): n_del + n_ins log rows"""
    for s, d, w in rows[:n_del]:
        r.x("DELETE FROM e WHERE rowid = (SELECT min(rowid) FROM e WHERE s = ? AND d = ? AND w = ?)", (s, d, w))
    r.many("INSERT INTO e VALUES (?, ?, ?)", [(f"n{i}", f"{tag}{i}" if i % 3 == 0 else f"n{i + 1}", 0.5 + i) for i in range(n_ins)])
    r.x("SELECT count(*) FROM g_delta")


def thresholds_small(r):
    """20 edges: a log of 10 rows is merged, one of 11 rebuilds in full (max(10, edge_count / 10)); a merge appends new nodes
    and swaps the last entry into a deleted one's place, a full rebuild renumbers and reorders, so the dumps tell which ran"""
    rows = _ring(10, 2, 5)
    r.x("CREATE TABLE e(s TEXT, d TEXT, w REAL)")
    r.many("INSERT INTO e VALUES (?, ?, ?)", rows)
    r.x(WEIGHTED)
    _changes(r, rows[::3], 5, 5, "x")
    r.x("SELECT count(*) FROM g")
    r.dump()
    _changes(r, rows[1::3], 5, 6, "y")
    r.x("SELECT count(*) FROM g")
    r.dump()


def thresholds_larger(r):
    """250 edges: edge_count / 10 = 25 log rows are merged, 26 rebuild in full"""
    rows = _ring(50, 5, 6)
    r.x("CREATE TABLE e(s TEXT, d TEXT, w REAL)")
    r.many("INSERT INTO e VALUES (?, ?, ?)", rows)
    r.x(WEIGHTED)
    r.x("SELECT value FROM g_config WHERE key = 'edge_count'")
    _changes(r, rows[::7], 12, 13, "x")
    r.x("SELECT count(*) FROM g")
    r.dump()
    r.x("SELECT value FROM g_config WHERE key = 'edge_count'")
    _changes(r, rows[1::7], 13, 13, "y")
    r.x("SELECT count(*) FROM g")
    r.dump()


def _chain(n):
    return [(f"n{i}", f"n{i + 1}", 1.0 + (i % 7) * 0.5) for i in range(n - 1)]


def nodes_4096_then_one_more(r):
    """exactly one full block; then a merge whose new node opens block 1"""
    r.x("CREATE TABLE e(s TEXT, d TEXT, w REAL)")
    r.many("INSERT INTO e VALUES (?, ?, ?)", _chain(4096) + [("n4095", "n0", 2.0), ("n7", "n4000", 0.5)])
    r.x(WEIGHTED)
    r.dump()
    r.x("SELECT * FROM g WHERE node IN ('n0', 'n4095', 'n4000')")
    r.x("INSERT INTO e VALUES ('n5', 'fresh', 3.0), ('fresh', 'n4095', 1.0), ('n4095', 'n5', 0.25)")
    r.x("INSERT INTO g(g) VALUES ('incremental_rebuild')")
    r.dump()
    r.x("SELECT * FROM g WHERE node IN ('n5', 'n4095', 'fresh')")
    r.x("SELECT node, in_degree, out_degree FROM graph_degree WHERE edge_table='g' AND src_col='s' AND dst_col='d' AND node IN ('n5', 'fresh')")


def nodes_4097(r):
    """two blocks from a full rebuild, the second with one node"""
    r.x("CREATE TABLE e(s TEXT, d TEXT, w REAL)")
    r.many("INSERT INTO e VALUES (?, ?, ?)", _chain(4097) + [("n4096", "n1", 2.0)])
    r.x(WEIGHTED)
    r.dump()
    r.x("SELECT * FROM g WHERE node IN ('n0', 'n1', 'n4095', 'n4096')")
    r.x("DELETE FROM e WHERE s = 'n4096'")
    r.x("DELETE FROM e WHERE s = 'n4095'")
    r.x("SELECT count(*) FROM g")
    r.dump()


def empty_then_filled(r):
    r.x("CREATE TABLE e(s TEXT, d TEXT, w REAL)")
    r.x(WEIGHTED)
    r.dump()
    r.x("SELECT * FROM g")
    r.tvfs()
    r.many("INSERT INTO e VALUES (?, ?, ?)", SMALL[:4])
    r.x("SELECT * FROM g")
    r.dump()
    r.x("UPDATE g_config SET value = '0' WHERE key = 'generation'")  # generation 0 with a non-empty log: a full rebuild
    r.x("INSERT INTO e VALUES ('p', 'q', 1.0)")
    r.x("SELECT * FROM g")
    r.dump()


def rename_then_insert(r):
    r.x("CREATE TABLE e(s TEXT, d TEXT, w REAL)")
    r.many("INSERT INTO e VALUES (?, ?, ?)", SMALL)
    r.x(WEIGHTED)
    r.x("ALTER TABLE g RENAME TO h")
    r.dump("h")
    r.x("INSERT INTO e VALUES ('a', 'new', 1.0)")
    r.x("SELECT * FROM h")
    r.x("SELECT * FROM g")
    r.dump("h")
    r.tvfs("h")


def rollback_takes_generation_back(r):
    r.x("CREATE TABLE e(s TEXT, d TEXT, w REAL)")
    r.many("INSERT INTO e VALUES (?, ?, ?)", SMALL)
    r.x(WEIGHTED)
    r.x("BEGIN")
    r.x("INSERT INTO e VALUES ('a', 'gone', 1.0)")
    r.x("INSERT INTO g(g) VALUES ('rebuild')")
    r.x("SELECT value FROM g_config WHERE key = 'generation'")
    r.x("ROLLBACK")
    r.dump()
    r.tvfs()
    r.x("INSERT INTO g(g) VALUES ('rebuild')")  # the instance counts on from what it reached inside the transaction
    r.x("SELECT value FROM g_config WHERE key = 'generation'")
    r.x("SAVEPOINT sp")
    r.x("INSERT INTO e VALUES ('a', 'gone2', 1.0)")
    r.x("SELECT count(*) FROM g")
    r.x("ROLLBACK TO sp")
    r.x("RELEASE sp")
    r.dump()


def reopen_then_incremental(r):
    """needs a file: created, closed, reopened, continued"""
    r.x("CREATE TABLE e(s TEXT, d TEXT, w REAL)")
    r.many("INSERT INTO e VALUES (?, ?, ?)", SMALL)
    r.x(WEIGHTED)
    r.reopen()
    r.x("SELECT * FROM g")
    r.tvfs()
    r.x("INSERT INTO e VALUES ('a', 'late', 1.0), ('late', 'b', 2.0)")
    r.x("DELETE FROM e WHERE s = 'd'")
    r.reopen()
    r.x("INSERT INTO g(g) VALUES ('incremental_rebuild')")
    r.dump()
    r.tvfs()


def argument_errors(r):
    r.x("CREATE TABLE e(s TEXT, d TEXT, w REAL)")
    for args in ("", "edge_table='e'", "edge_table='e', src_col='s'", "src_col='s', dst_col='d'", "edge_table='e', src_col='s', dst_col='d', nope=1",
                 "nope", "edge_table='e e', src_col='s', dst_col='d'", "edge_table='e', src_col='s;', dst_col='d'",
                 "edge_table='e', src_col='s', dst_col=''", "edge_table='e', src_col='s', dst_col='d', weight_col='w w'",
                 "edge_table='missing', src_col='s', dst_col='d'", "edge_table='e', src_col='missing', dst_col='d'",
                 "edge_table='e', src_col='s', dst_col='d', weight_col='missing'", "edge_table=e, src_col=\"s\", dst_col='d', weight_col=w",
                 "edge_table='e', edge_table='e', src_col='s', dst_col='d'"):
        r.x(f"CREATE VIRTUAL TABLE g USING graph_adjacency({args})")
        r.x("SELECT name FROM sqlite_master WHERE name LIKE 'g%' ORDER BY name")
        r.x("DROP TABLE IF EXISTS g")


def empty_create_rename_drop(r):
    """nothing here reaches a device: the edge table stays empty"""
    r.x("CREATE TABLE e(s TEXT, d TEXT, w REAL)")
    r.x(WEIGHTED)
    r.dump()
    r.x("SELECT * FROM g")
    r.x("INSERT INTO g(g) VALUES ('rebuild')")
    r.x("INSERT INTO g(g) VALUES ('incremental_rebuild')")
    r.x("INSERT INTO g(g) VALUES ('stats')")
    r.x("INSERT INTO g(g) VALUES ('nope')")
    r.x("INSERT INTO g(g) VALUES (NULL)")
    r.x("INSERT INTO g(node) VALUES ('x')")
    r.x("INSERT INTO g(rowid, g) VALUES (1, 'rebuild')")
    r.dump()
    r.x("ALTER TABLE g RENAME TO h")
    r.dump("h")
    r.x("SELECT * FROM h")
    r.x("CREATE VIRTUAL TABLE g2 USING graph_adjacency(edge_table='e', src_col='s', dst_col='d')")
    r.dump("g2")
    r.x("DROP TABLE h")
    r.x("DROP TABLE g2")
    r.dump("h")
    r.x("SELECT name FROM sqlite_master ORDER BY name")


SESSIONS = {f.__name__: f for f in (empty_create_rename_drop, weighted_small, unweighted_integers, thresholds_small, thresholds_larger, nodes_4096_then_one_more,
                                    nodes_4097, empty_then_filled, rename_then_insert, rollback_takes_generation_back,
                                    reopen_then_incremental, argument_errors)}
NEEDS_FILE = {"reopen_then_incremental"}
# sessions in which every statement ends before any device call: an empty edge table, or no table at all
CPU_SESSIONS = ("argument_errors", "empty_create_rename_drop")


def run(name, load, tmpdir=None):
    path = os.path.join(tmpdir, name + ".db") if name in NEEDS_FILE else ":memory:"
    r = Recorder(load, path)
    try:
        SESSIONS[name](r)
    finally:
        r.close()
    return r.out
