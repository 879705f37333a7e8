#!/usr/bin/env python3
"""graph_select on one MI355X: mn_graph_select over the 1M-node / 20M-edge Barabasi-Albert graph of bench_graph.py (the
graph of bench_bfs.py) and over a path.

  (a) `x+`, `+x+`, `@x` without limits from one fixed node, and a union of ten terms: wall ms, device ms, levels and status
      read-backs, each with the bottom-up step forced off, forced on and chosen per level (MN_SELECT_BOTTOM_UP = 0, 1, auto)
  (b) `x+` with the per-level choice at several thresholds (MN_SELECT_BOTTOM_UP_DIV): where the switch point lies
  (c) next to `x+`, the only way to the same rows without graph_select: Graph.bfs(x, unlimited, 'forward') and a host sort
      by node — same graph, same process, the two interleaved — and the ratio of the two wall times
  (d) a path of --path-nodes nodes from its first node: µs per level with 1, 4, 8, 16 and 32 levels queued per status
      read-back (MN_SELECT_LEVELS_PER_SYNC), next to graph_bfs on the same path

The rows are first checked against tests/select_model.py (the reference's evaluator in plain Python, itself held to the
reference's recorded rows by tests/test_select_model.py) on a --check-nodes graph built the same way.  Medians of --runs runs
in one process; one JSON line, also written to --out.

  python bench_select.py --out profiles/select_1M_20M.json
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

from bench_graph import ba_edges  # noqa: E402

ENV = ("MN_SELECT_BOTTOM_UP", "MN_SELECT_BOTTOM_UP_DIV", "MN_SELECT_LEVELS_PER_SYNC")
MODES = ("0", "1", "auto")


def index_of(name):
    return int(name[1:]) if name[:1] == b"n" and name[1:].isdigit() else -1


def setenv(**kw):
    for k in ENV:
        os.environ.pop(k, None)
    for k, v in kw.items():
        if v is not None:
            os.environ["MN_SELECT_" + k] = str(v)


def queries(n):
    x = n // 2
    rng = np.random.default_rng(3)
    t = rng.integers(0, n, 10).tolist()
    union = (f"n{t[0]}+1 n{t[1]}+2 +n{t[2]} 2+n{t[3]} 1+n{t[4]}+1 @n{t[5]} n{t[6]}+,+n{t[7]} not n{t[8]}+1 n{t[9]} n{x}+")
    return {"descendants": f"n{x}+", "both": f"+n{x}+", "closure": f"@n{x}", "union_of_ten": union}


def check_against_model(pkg, n, m):
    import select_model as sm

    src, dst = ba_edges(n, m)
    g = pkg.graph.graph_from_edges(n, src, dst)
    lists = sm.lists_of(n, src, dst)
    for name, expr in queries(n).items():
        rows, direction = sm.evaluate(sm.parse(expr), n, lists[0], lists[1], index_of)
        for mode in MODES:
            setenv(BOTTOM_UP=mode)
            node, depth, d = g.select(expr, names=index_of)
            assert (node.tolist(), depth.tolist(), d) == ([r[0] for r in rows], [r[1] for r in rows], direction), \
                f"bench_select: the device's rows for {name} (bottom-up {mode}) differ from the model's"
    setenv()
    g.close()
    return {"nodes": n, "edges": int(len(src)), "queries": sorted(queries(n)), "modes": list(MODES), "rows_equal_model": True}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=1_000_000)
    ap.add_argument("--attach", type=int, default=20, help="edges per arriving node (20 → 20M edges at 1M nodes)")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--path-nodes", type=int, default=20_000)
    ap.add_argument("--check-nodes", type=int, default=100_000)
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    import muninn_amd

    pkg = muninn_amd.pkg
    pkg.build()
    pkg.lib()
    assert pkg.device_count() >= 1, "bench_select: no gfx950 device"
    checked = check_against_model(pkg, args.check_nodes, args.attach)
    src, dst = ba_edges(args.nodes, args.attach)
    g = pkg.graph.graph_from_edges(args.nodes, src, dst)
    med = statistics.median

    def timed(fn, stats):
        t0 = time.perf_counter()
        r = fn()
        return (time.perf_counter() - t0) * 1e3, r, dict(stats())

    def select_runs(expr, runs=args.runs):
        g.select(expr, names=index_of)  # warm-up: the first call allocates the scratch
        rs = [timed(lambda: g.select(expr, names=index_of), lambda: g.select_stats) for _ in range(runs)]
        st = rs[0][2]
        return {"ms": med(r[0] for r in rs), "device_ms": med(r[2]["device_ms"] for r in rs), "rows": st["rows"], "levels": st["levels"],
                "bottom_up_levels": st["bottom_up_levels"], "launches": st["launches"], "syncs": st["syncs"]}

    qs = queries(args.nodes)
    by_query = {}
    for name, expr in qs.items():
        by_query[name] = {"selector": expr}
        for mode in MODES:
            setenv(BOTTOM_UP=mode)
            by_query[name]["bottom_up_" + mode] = select_runs(expr)
    switch = {}
    for div in (1, 2, 4, 8, 16, 32, 64, 256, 1024):
        setenv(BOTTOM_UP="auto", BOTTOM_UP_DIV=div)
        switch[str(div)] = {k: select_runs(qs[k]) for k in ("descendants", "closure")}
    setenv()

    # the same rows without graph_select: the traversal's rows in queue order, sorted by node on the host
    x = args.nodes // 2

    def bfs_route():
        node, depth, _ = g.bfs(x, 2**31 - 1, "forward")
        o = np.argsort(node, kind="stable")
        return node[o], depth[o]

    want = g.select(qs["descendants"], names=index_of)
    got = bfs_route()
    assert np.array_equal(want[0], got[0]) and np.array_equal(want[1], got[1]), "bench_select: graph_bfs + sort gives other rows"
    a, b = [], []
    for _ in range(args.runs):
        a.append(timed(lambda: g.select(qs["descendants"], names=index_of), lambda: g.select_stats))
        b.append(timed(bfs_route, lambda: g.bfs_stats))
    sel_ms, bfs_ms = med(r[0] for r in a), med(r[0] for r in b)
    versus = {"selector": qs["descendants"], "rows": int(len(want[0])), "graph_select_ms": sel_ms, "graph_select_device_ms": med(r[2]["device_ms"] for r in a),
              "graph_bfs_plus_host_sort_ms": bfs_ms, "graph_bfs_device_ms": med(r[2]["device_ms"] for r in b),
              "graph_bfs_levels": b[0][2]["levels"], "bfs_route_over_select": bfs_ms / sel_ms}
    g.close()

    n = args.path_nodes
    g = pkg.graph.graph_from_edges(n, np.arange(n - 1), np.arange(1, n))
    path = {"nodes": n, "levels_per_sync": {}}
    for lps in (1, 4, 8, 16, 32):
        setenv(LEVELS_PER_SYNC=lps)
        node, depth, _ = g.select("n0+", names=index_of)
        assert np.array_equal(node, np.arange(n)) and np.array_equal(depth, np.arange(n))
        r = select_runs("n0+")
        path["levels_per_sync"][str(lps)] = dict(r, us_per_level=r["ms"] * 1e3 / r["levels"], device_us_per_level=r["device_ms"] * 1e3 / r["levels"])
    setenv()
    g.bfs(0, 2**31 - 1, "forward")
    rs = [timed(lambda: g.bfs(0, 2**31 - 1, "forward"), lambda: g.bfs_stats) for _ in range(args.runs)]
    wall, levels = med(r[0] for r in rs), rs[0][2]["levels"]
    path["graph_bfs"] = {"ms": wall, "device_ms": med(r[2]["device_ms"] for r in rs), "levels": levels, "us_per_level": wall * 1e3 / levels}
    g.close()

    res = {"workload": "graph_select", "graph": {"model": "barabasi-albert", "nodes": args.nodes, "edges": int(len(src))},
           "runs": args.runs, "queries": by_query, "auto_threshold_divisor": switch, "descendants_versus_graph_bfs": versus,
           "path_one_entry_per_level": path, "checked_against_model": checked}
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
