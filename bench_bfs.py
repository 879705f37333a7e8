#!/usr/bin/env python3
"""graph_bfs on one MI355X: mn_graph_bfs over the 1M-node / 20M-edge Barabasi-Albert graph of bench_graph.py.

  (a) one seed, direction 'both', unlimited depth: ms, levels, list entries scanned per second, and the mean host round
      trip per level = (wall - device) / levels — every level costs one
  (b) 10 000 seeds, 'forward', max_depth 2, in one call: ms, rows per second, chunks — and the same seeds as 10 000 calls
  (c) a path of --path-nodes nodes from its first node: as many levels as nodes, one entry each — what a level costs when
      there is nothing in it: wall and device time per level

Each answer is first checked, row for row, against tests/bfs_model.py (the queue BFS in plain Python, itself held to the
reference's recorded rows by tests/test_bfs_model.py) on a --check-nodes subgraph built the same way: the model would take
minutes on the full graph.  Medians of --runs runs in one process; one JSON line, also written to --out.

  python bench_bfs.py --out profiles/bfs_1M_20M.json
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


def check_against_model(pkg, n, m, n_seeds):
    import bfs_model as bm

    src, dst = ba_edges(n, m)
    g = pkg.graph.graph_from_edges(n, src, dst)
    out, inn = bm.lists_of(n, src, dst)
    seeds = np.random.default_rng(1).integers(0, n, n_seeds)
    for got, want in ((g.bfs_batch(seeds[:1], 2**31 - 1, "both"), bm.bfs_arrays(out, inn, seeds[:1], 2**31 - 1, "both")),
                      (g.bfs_batch(seeds, 2, "forward"), bm.bfs_arrays(out, inn, seeds, 2, "forward"))):
        assert all(np.array_equal(a, b) for a, b in zip(got, want)), "bench_bfs: the device's rows differ from the model's"
    g.close()
    return {"nodes": n, "edges": int(len(src)), "seeds": int(n_seeds), "rows_equal_model": True}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=1_000_000)
    ap.add_argument("--attach", type=int, default=20, help="edges per arriving node (20 → 20M edges at 1M nodes)")
    ap.add_argument("--seeds", type=int, default=10_000)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--path-nodes", type=int, default=20_000)
    ap.add_argument("--check-nodes", type=int, default=100_000)
    ap.add_argument("--check-seeds", type=int, default=500)
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    import muninn_amd

    pkg = muninn_amd.pkg
    pkg.build()
    pkg.lib()
    assert pkg.device_count() >= 1, "bench_bfs: no gfx950 device"
    checked = check_against_model(pkg, args.check_nodes, args.attach, args.check_seeds)
    src, dst = ba_edges(args.nodes, args.attach)
    g = pkg.graph.graph_from_edges(args.nodes, src, dst)
    seeds = np.random.default_rng(2).integers(0, args.nodes, args.seeds)
    med = statistics.median

    def timed(fn):
        t0 = time.perf_counter()
        r = fn()
        return (time.perf_counter() - t0) * 1e3, r, dict(g.bfs_stats)

    g.bfs(int(seeds[0]), 2**31 - 1, "both")  # warm-up: scratch allocation, the visited words' one fill
    one = [timed(lambda: g.bfs(int(seeds[0]), 2**31 - 1, "both")) for _ in range(args.runs)]
    st = one[0][2]
    wall, dev = med(r[0] for r in one), med(r[2]["device_ms"] for r in one)
    single = {"ms": wall, "device_ms": dev, "rows": st["rows"], "levels": st["levels"], "edges_scanned": st["edges_scanned"],
              "edges_scanned_per_s": st["edges_scanned"] / (wall * 1e-3), "round_trip_us_per_level": (wall - dev) * 1e3 / st["levels"]}

    g.bfs_batch(seeds, 2, "forward")
    many = [timed(lambda: g.bfs_batch(seeds, 2, "forward")) for _ in range(args.runs)]
    st = many[0][2]
    wall = med(r[0] for r in many)
    batch = {"ms": wall, "device_ms": med(r[2]["device_ms"] for r in many), "rows": st["rows"], "chunks": st["chunks"],
             "levels": st["levels"], "edges_scanned": st["edges_scanned"], "rows_per_s": st["rows"] / (wall * 1e-3)}

    def singles():
        rows = 0
        for s in seeds.tolist():
            rows += len(g.bfs(s, 2, "forward")[0])
        return rows

    loop = [timed(singles) for _ in range(args.runs)]
    assert loop[0][1] == batch["rows"]
    wall = med(r[0] for r in loop)
    batch["as_single_calls"] = {"ms": wall, "rows_per_s": batch["rows"] / (wall * 1e-3), "ms_per_call": wall / len(seeds)}
    g.close()

    n = args.path_nodes
    g = pkg.graph.graph_from_edges(n, np.arange(n - 1), np.arange(1, n))
    node = g.bfs(0, 2**31 - 1, "forward")[0]
    assert np.array_equal(node, np.arange(n))
    runs = [timed(lambda: g.bfs(0, 2**31 - 1, "forward")) for _ in range(args.runs)]
    st = runs[0][2]
    wall, dev = med(r[0] for r in runs), med(r[2]["device_ms"] for r in runs)
    path = {"nodes": n, "levels": st["levels"], "ms": wall, "device_ms": dev, "us_per_level": wall * 1e3 / st["levels"],
            "device_us_per_level": dev * 1e3 / st["levels"], "round_trip_us_per_level": (wall - dev) * 1e3 / st["levels"]}
    g.close()
    res = {"workload": "graph_bfs", "graph": {"model": "barabasi-albert", "nodes": args.nodes, "edges": int(len(src))},
           "runs": args.runs, "one_seed_both_unlimited": single, "batch_forward_depth2": dict(batch, seeds=args.seeds),
           "path_one_entry_per_level": path,
           "checked_against_model": checked}
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
