#!/usr/bin/env python3
"""graph_dfs on one MI355X: mn_graph_dfs over the 1M-node / 20M-edge Barabasi-Albert graph of bench_graph.py.

  (a) one seed, 'forward', unlimited depth: wall and device ms, rows per second, list entries scanned, most frames at once —
      one wavefront, one latency chain
  (b) 10 000 seeds (those of bench_bfs.py), 'forward', max_depth 2, in one call: ms, rows per second, chunks — and the same
      seeds as 10 000 calls
  (c) 2 000 seeds, 'forward', max_depth 100, in one call on the --check-nodes graph: thousands of long chains side by side
  (d) where the compiled reference is on the box (oracle/_ref/muninn.so): its graph_dfs and ours through SQL on a
      --sql-nodes graph, both tables indexed on either column, rows compared

Each answer is first checked, row for row, against tests/dfs_model.py (the reference's item stack in plain Python, itself held
to the reference's recorded rows by tests/test_dfs_model.py) on the --check-nodes graph: the model would take minutes on the
full one.  Medians of --runs runs in one process; one JSON line, also written to --out.

  python bench_dfs.py --out profiles/dfs_1M_20M.json
"""
import argparse
import json
import os
import sqlite3
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

from bench_graph import ba_edges  # noqa: E402

UNLIMITED = 2**31 - 1


def check_against_model(g, n, src, dst, n_seeds, n_deep):
    import dfs_model as dm

    out, inn = dm.lists_of(n, src, dst)
    seeds = np.random.default_rng(1).integers(0, n, n_seeds)
    for s, depth in ((seeds[:1], UNLIMITED), (seeds, 2), (seeds[:n_deep], 100)):
        got, want = g.dfs_batch(s, depth, "forward"), dm.dfs_arrays(out, inn, s, depth, "forward")
        assert all(np.array_equal(a, b) for a, b in zip(got, want)), "bench_dfs: the device's rows differ from the model's"
    return {"nodes": n, "edges": int(len(src)), "seeds_depth_2": int(n_seeds), "seeds_depth_100": int(n_deep), "rows_equal_model": True}


def sql_leg(n, m, runs):
    """the reference's graph_dfs and ours on the same table through sqlite3, one start node, forward, to the end"""
    from oracle import orc_graph as og

    if not og.have_ref_graph():
        return None
    src, dst = ba_edges(n, m)
    rows = [(f"n{a}", f"n{b}") for a, b in zip(src.tolist(), dst.tolist())]
    sql = f"SELECT node, depth, parent FROM graph_dfs('e', 's', 'd', 'n{n - 1}', {UNLIMITED}, 'forward')"
    res, answers = {"nodes": n, "rows_in_table": len(rows)}, []
    for who, path in (("reference", og.REF_EXT_SO[:-3]), ("ours", os.path.join(ROOT, "sqlite-muninn_amd", "ext", "muninn"))):
        c = sqlite3.connect(":memory:")
        c.enable_load_extension(True)
        c.load_extension(path)
        c.execute("CREATE TABLE e(s TEXT, d TEXT)")
        c.executemany("INSERT INTO e VALUES (?, ?)", rows)
        c.execute("CREATE INDEX e_s ON e(s)")
        c.execute("CREATE INDEX e_d ON e(d)")
        c.commit()
        got = c.execute(sql).fetchall()  # warm-up
        ms = []
        for _ in range(runs):
            t0 = time.perf_counter()
            got = c.execute(sql).fetchall()
            ms.append((time.perf_counter() - t0) * 1e3)
        answers.append(got)
        res[who] = {"ms": statistics.median(ms), "rows": len(got)}
        c.close()
    assert answers[0] == answers[1], "bench_dfs: graph_dfs's rows differ from the reference's"
    res["rows_equal_reference"] = True
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=1_000_000)
    ap.add_argument("--attach", type=int, default=20, help="edges per arriving node (20 → 20M edges at 1M nodes)")
    ap.add_argument("--seeds", type=int, default=10_000)
    ap.add_argument("--deep-seeds", type=int, default=2_000)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--check-nodes", type=int, default=100_000)
    ap.add_argument("--check-seeds", type=int, default=500)
    ap.add_argument("--check-deep-seeds", type=int, default=8)
    ap.add_argument("--sql-nodes", type=int, default=10_000)
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    import muninn_amd

    pkg = muninn_amd.pkg
    pkg.build()
    pkg.lib()
    assert pkg.device_count() >= 1, "bench_dfs: no gfx950 device"
    med = statistics.median

    def timed(g, fn):
        t0 = time.perf_counter()
        r = fn()
        return (time.perf_counter() - t0) * 1e3, r, dict(g.dfs_stats)

    def leg(g, seeds, max_depth):
        g.dfs_batch(seeds, max_depth, "forward")  # warm-up: the scratch of this shape
        runs = [timed(g, lambda: g.dfs_batch(seeds, max_depth, "forward")) for _ in range(args.runs)]
        st, wall = runs[0][2], med(r[0] for r in runs)
        return {"seeds": len(seeds), "max_depth": max_depth, "ms": wall, "device_ms": med(r[2]["device_ms"] for r in runs),
                "rows": st["rows"], "chunks": st["chunks"], "entries_scanned": st["entries_scanned"], "max_frames": st["max_frames"],
                "rows_per_s": st["rows"] / (wall * 1e-3), "us_per_row": wall * 1e3 / max(st["rows"], 1)}

    # the small graph: the check, and the long chains side by side
    cs, cd = ba_edges(args.check_nodes, args.attach)
    g = pkg.graph.graph_from_edges(args.check_nodes, cs, cd)
    checked = check_against_model(g, args.check_nodes, cs, cd, args.check_seeds, args.check_deep_seeds)
    deep = leg(g, np.random.default_rng(3).integers(0, args.check_nodes, args.deep_seeds), 100)
    deep["nodes"] = args.check_nodes
    g.close()

    src, dst = ba_edges(args.nodes, args.attach)
    g = pkg.graph.graph_from_edges(args.nodes, src, dst)
    seeds = np.random.default_rng(2).integers(0, args.nodes, args.seeds)
    single = leg(g, seeds[:1], UNLIMITED)
    batch = leg(g, seeds, 2)

    def singles():
        rows = 0
        for s in seeds.tolist():
            rows += len(g.dfs(s, 2, "forward")[0])
        return rows

    loop = [timed(g, singles) for _ in range(args.runs)]
    assert loop[0][1] == batch["rows"]
    wall = med(r[0] for r in loop)
    batch["as_single_calls"] = {"ms": wall, "rows_per_s": batch["rows"] / (wall * 1e-3), "ms_per_call": wall / len(seeds)}
    g.close()

    res = {"workload": "graph_dfs", "graph": {"model": "barabasi-albert", "nodes": args.nodes, "edges": int(len(src))},
           "runs": args.runs, "one_seed_forward_unlimited": single, "batch_forward_depth2": batch,
           "batch_forward_depth100_small_graph": deep, "sql_against_reference": sql_leg(args.sql_nodes, args.attach, args.runs),
           "checked_against_model": checked}
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
