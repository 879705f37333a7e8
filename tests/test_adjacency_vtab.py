"""The graph_adjacency virtual table of ext/muninn.so (ext/mn_adjacency_vtab.c) against the reference's.

tests/golden/adjacency_vtab.json.gz holds the sessions of tests/adjacency_sessions.py as the REFERENCE's extension answered
them (scripts/gen_adjacency_golden.py): statement by statement rows or error text, and at every checkpoint the six shadow
tables, the trigger rows of sqlite_master and pragma_table_xinfo.  The same sessions through this extension must give the same
transcript, with the device copy kept between statements and with MUNINN_ADJ_RESIDENT=0.  Where the compiled reference
travels with the tree, larger random sessions and both directions of file interchange are compared live."""
import gzip
import json
import os
import sqlite3
import subprocess

import numpy as np
import pytest

import adjacency_sessions as sess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXT = os.path.join(ROOT, "sqlite-muninn_amd", "ext", "muninn")
REF = os.path.join(ROOT, "oracle", "_ref", "muninn")
WEIGHTED = sess.WEIGHTED.replace("'e'", "'edges'").replace("'s'", "'src'").replace("'d'", "'dst'").replace("'w'", "'weight'")


@pytest.fixture(scope="module")
def golden():
    with gzip.open(os.path.join(ROOT, "tests", "golden", "adjacency_vtab.json.gz"), "rt") as f:
        return json.load(f)


@pytest.fixture(scope="module")
def ext(mn):
    mn.build()
    subprocess.run(["make", "-s", "-C", os.path.dirname(EXT)], check=True)
    return lambda c: c.load_extension(EXT)


def same_transcript(got, want):
    got = json.loads(json.dumps(got))  # tuples → lists, as the recording went through JSON
    for i, (a, b) in enumerate(zip(got, want)):
        assert a == b, f"line {i}: ours {str(a)[:600]} reference {str(b)[:600]}"
    assert len(got) == len(want)


def connect(load, path=":memory:"):
    c = sqlite3.connect(path, isolation_level=None)
    c.enable_load_extension(True)
    load(c)
    return c


# ───────────────────────── without a device ─────────────────────────

def test_module_and_function_are_registered(ext):
    c = connect(ext)
    assert "graph_adjacency" in {r[0] for r in c.execute("SELECT name FROM pragma_module_list")}
    assert c.execute("SELECT count(*) FROM pragma_function_list WHERE name='muninn_adjacency_resident' AND narg=1").fetchone()[0] == 1
    c.execute("CREATE TABLE e(s TEXT, d TEXT, w REAL)")
    c.execute(sess.WEIGHTED)
    assert c.execute("SELECT muninn_adjacency_resident('g'), muninn_adjacency_resident('nope'), muninn_adjacency_resident(NULL)").fetchall() == \
        [(None, None, None)]  # an empty graph has no device copy
    c.close()


@pytest.mark.parametrize("name", sess.CPU_SESSIONS)
def test_sessions_that_need_no_device_equal_the_recording(ext, golden, tmp_path, name):
    """argument errors, command errors, creating over an empty edge table (shadow tables, trigger text, config rows), rename, drop"""
    same_transcript(sess.run(name, ext, str(tmp_path)), golden[name])


def test_the_recording_holds_the_cases_it_is_there_for(golden):
    assert set(golden) == set(sess.SESSIONS)
    dumps = {n: [line for line in t if isinstance(line, dict)] for n, t in golden.items()}
    assert [len(d["_csr_fwd"]) for d in dumps["nodes_4096_then_one_more"]] == [1, 2]
    assert len(dumps["nodes_4097"][0]["_csr_rev"]) == 2
    assert any("no such column: NEW.NULL" in str(line) for line in golden["unweighted_integers"])
    assert 'NEW."NULL"' in str(dumps["unweighted_integers"][0]["triggers"])


# ───────────────────────── on the GPU ─────────────────────────

@pytest.mark.gpu
@pytest.mark.parametrize("resident", [None, "0"])
@pytest.mark.parametrize("name", sorted(sess.SESSIONS))
def test_every_recorded_session_replays_to_the_same_transcript(gpu, ext, golden, tmp_path, monkeypatch, name, resident):
    monkeypatch.setenv("MUNINN_GRAPH_MODE", "exact")
    if resident is None:
        monkeypatch.delenv("MUNINN_ADJ_RESIDENT", raising=False)
    else:
        monkeypatch.setenv("MUNINN_ADJ_RESIDENT", resident)
    same_transcript(sess.run(name, ext, str(tmp_path)), golden[name])


def need_ref():
    if not os.path.exists(REF + ".so"):
        pytest.skip("oracle/_ref/muninn.so (the compiled reference) is not present")
    return lambda c: c.load_extension(REF)


def dump(c, t="g"):
    out = {s: c.execute(f'SELECT * FROM "{t}{s}" ORDER BY 1').fetchall() for s in sess.SHADOWS}
    out["rows"] = c.execute(f'SELECT * FROM "{t}" ORDER BY node_idx').fetchall()
    out["triggers"] = c.execute("SELECT name, tbl_name, sql FROM sqlite_master WHERE type='trigger' ORDER BY name").fetchall()
    return out


def same_dump(got, want):
    for k in want:
        assert len(got[k]) == len(want[k]) and got[k] == want[k], k


def random_parts(seed):
    rng = np.random.default_rng(seed)
    n, m = 5000, 14000
    s0, d0 = rng.integers(0, n, m), rng.integers(0, n, m)
    w0 = rng.integers(1, 13, m) * 0.25
    base = [(f"n{a}", f"n{b}", float(x)) for a, b, x in zip(s0, d0, w0)]
    ins = [(f"n{int(a)}", f"n{int(b)}" if i % 5 else f"new{int(b) % 40}", float(x))
           for i, (a, b, x) in enumerate(zip(rng.integers(0, n, 300), rng.integers(0, n, 300), rng.integers(1, 9, 300) * 0.5))]
    dele = [(f"n{s0[i]}", f"n{d0[i]}") for i in rng.permutation(m)[:250]]
    return base, ins, dele


def fill(c, base):
    c.execute("CREATE TABLE edges (src TEXT, dst TEXT, weight REAL)")
    c.execute("BEGIN")
    c.executemany("INSERT INTO edges VALUES (?,?,?)", base)
    c.execute("COMMIT")
    c.execute(WEIGHTED)


def change(c, ins, dele):
    c.execute("BEGIN")
    c.executemany("DELETE FROM edges WHERE src = ? AND dst = ?", dele)
    c.executemany("INSERT INTO edges VALUES (?,?,?)", ins)
    c.execute("COMMIT")


@pytest.mark.gpu
@pytest.mark.parametrize("seed", [41, 42])
def test_random_sessions_at_5000_nodes_equal_the_reference_live(gpu, ext, seed):
    """two CSR blocks; a full rebuild, then deletes and inserts (new nodes among them) merged incrementally, then a log past
    the tenth of the edges, which a SELECT rebuilds in full: the dumps after each step are equal"""
    ref = need_ref()
    base, ins, dele = random_parts(seed)

    def session(load):
        c = connect(load)
        fill(c, base)
        out = [dump(c)]
        change(c, ins, dele)
        assert c.execute("SELECT count(*) FROM g_delta").fetchone()[0] >= 500
        c.execute("INSERT INTO g(g) VALUES ('incremental_rebuild')")
        out.append(dump(c))
        c.execute("BEGIN")
        c.executemany("INSERT INTO edges VALUES (?,?,?)", [(f"m{i}", f"n{i}", 1.0) for i in range(1500)])
        c.execute("COMMIT")
        out.append(dump(c))  # its SELECT refreshes: more than edge_count / 10 log rows
        c.close()
        return out

    for got, want in zip(session(ext), session(ref)):
        same_dump(got, want)


@pytest.mark.gpu
@pytest.mark.parametrize("creator", ["ours", "reference"])
def test_a_file_made_by_one_extension_continues_under_the_other(gpu, ext, tmp_path, creator):
    ref = need_ref()
    base, ins, dele = random_parts(7)
    loaders = {"ours": ext, "reference": ref}

    def session(first, second, path):
        c = connect(first, path)
        fill(c, base)
        c.close()
        c = connect(second, path)
        change(c, ins, dele)
        c.execute("INSERT INTO g(g) VALUES ('incremental_rebuild')")
        out = dump(c)
        c.close()
        return out

    want = session(ref, ref, str(tmp_path / "all_reference.db"))
    other = "reference" if creator == "ours" else "ours"
    same_dump(session(loaders[creator], loaders[other], str(tmp_path / "mixed.db")), want)


DEGREE = "SELECT * FROM graph_degree WHERE edge_table='{t}' AND src_col='s' AND dst_col='d'"
RESIDENT = "SELECT muninn_adjacency_resident('{t}')"


def small(ext):
    c = connect(ext)
    c.execute("CREATE TABLE e(s TEXT, d TEXT, w REAL)")
    c.executemany("INSERT INTO e VALUES (?, ?, ?)", sess.SMALL)
    c.execute(sess.WEIGHTED)
    return c


@pytest.mark.gpu
def test_the_graph_stays_on_the_device_between_statements(gpu, ext, monkeypatch, tmp_path):
    monkeypatch.delenv("MUNINN_ADJ_RESIDENT", raising=False)
    c = small(ext)
    res = lambda t="g": c.execute(RESIDENT.format(t=t)).fetchone()[0]  # noqa: E731
    deg = lambda t="g": c.execute(DEGREE.format(t=t)).fetchall()  # noqa: E731
    plain = lambda: c.execute(DEGREE.format(t="e") + " AND weight_col='w'").fetchall()  # noqa: E731
    assert res() == 1  # the full rebuild of CREATE left its graph behind
    fresh = deg()
    assert fresh == plain() and res() == 1
    c.execute("INSERT INTO e VALUES ('a', 'z', 9.0), ('z', 'b', 0.5)")
    assert c.execute("SELECT count(*) FROM g_delta").fetchone()[0] == 2
    stale = deg()  # a non-empty log: the edge table is read, as the reference does
    assert stale == plain() and stale != fresh and c.execute("SELECT count(*) FROM g_delta").fetchone()[0] == 2
    c.execute("INSERT INTO g(g) VALUES ('incremental_rebuild')")
    assert res() is None  # the device copy was of the state before the merge
    merged = deg()
    assert sorted(merged) == sorted(stale) and res() == 2  # loaded from the stored blocks and kept
    assert deg() == merged and res() == 2
    c.execute("INSERT INTO g(g) VALUES ('rebuild')")
    assert res() == 3 and sorted(deg()) == sorted(stale)
    before = deg()
    c.execute("BEGIN")
    c.execute("INSERT INTO e VALUES ('a', 'gone', 1.0)")
    c.execute("INSERT INTO g(g) VALUES ('rebuild')")
    assert res() == 4 and len(deg()) == len(before) + 1
    c.execute("ROLLBACK")
    assert res() is None
    assert deg() == before and res() == 3  # the rows of the rolled-back state, loaded again under its generation
    c.execute("ALTER TABLE g RENAME TO h")
    assert res("g") is None and res("h") is None
    assert deg("h") == before and res("h") == 3
    c.execute("DROP TABLE h")
    assert res("h") is None
    c.close()
    # a file: nothing is resident after reopening until the first call
    path = str(tmp_path / "r.db")
    c = connect(ext, path)
    c.execute("CREATE TABLE e(s TEXT, d TEXT, w REAL)")
    c.executemany("INSERT INTO e VALUES (?, ?, ?)", sess.SMALL)
    c.execute(sess.WEIGHTED)
    want = c.execute(DEGREE.format(t="g")).fetchall()
    c.close()
    c = connect(ext, path)
    assert c.execute(RESIDENT.format(t="g")).fetchone()[0] is None
    assert c.execute(DEGREE.format(t="g")).fetchall() == want
    assert c.execute(RESIDENT.format(t="g")).fetchone()[0] == 1
    other = connect(ext, path)  # another connection commits: this one's copy is no longer trusted
    other.execute("INSERT INTO e VALUES ('x', 'y', 1.0)")
    other.execute("INSERT INTO g(g) VALUES ('rebuild')")
    other.close()
    assert c.execute(RESIDENT.format(t="g")).fetchone()[0] is None
    assert len(c.execute(DEGREE.format(t="g")).fetchall()) == len(want) + 2
    c.close()


@pytest.mark.gpu
def test_residency_switched_off_changes_no_row(gpu, ext, monkeypatch):
    rows = {}
    for setting in (None, "0"):
        if setting is None:
            monkeypatch.delenv("MUNINN_ADJ_RESIDENT", raising=False)
        else:
            monkeypatch.setenv("MUNINN_ADJ_RESIDENT", setting)
        c = small(ext)
        got = [c.execute(RESIDENT.format(t="g")).fetchone()[0]]
        for f in ("graph_degree", "graph_closeness", "graph_node_betweenness"):
            for _ in range(2):
                got.append(c.execute(f"SELECT * FROM {f} WHERE edge_table='g' AND src_col='s' AND dst_col='d'").fetchall())
        got.append(c.execute("SELECT node, community_id, modularity FROM graph_leiden WHERE edge_table='g' AND src_col='s' AND dst_col='d'").fetchall())
        rows[setting] = got
        c.close()
    assert rows[None][0] == 1 and rows["0"][0] is None
    assert rows[None][1:] == rows["0"][1:]
