#!/usr/bin/env python3
"""graph_shortest_path on one MI355X: mn_graph_shortest_paths over the 1M-node / 20M-edge Barabasi-Albert graph of
bench_bfs.py (forward lists: a node's edges lead to older nodes) with seeded uniform (0, 1] f64 weights.

  (a) one pair in fast mode: wall and kernel ms, relaxations, passes, relaxations per second
  (b) --pairs pairs over --starts distinct starts in one call, and the first --loop-pairs of them sent one call each
  (c) (a)'s pair and (b)'s call under five values of MN_SSSP_DELTA
  (d) replay on --replay-nodes nodes / --replay-rows rows, and on a 10th, 20th, 50th and 100th of that: --replay-pairs pairs
      and one pair, against fast mode on the same pairs (where replay stops being the faster of the two is where
      MN_SP_AUTO stops choosing it), and at the full size — where oracle/_ref/muninn.so is present — against the compiled
      reference's graph_shortest_path on the same table: the rows must be equal, and both times are printed

Half of the ends are drawn from the oldest 1 000 nodes, which every start reaches; the other half from all nodes, most of
which a start does not reach, so that their search runs until nothing is pending.  Each answer is first checked against
tests/sp_model.py (itself held to the reference's recorded rows by tests/test_sp_model.py) on a --check-nodes graph built
the same way.  Medians of --runs runs in one process; one JSON line, also written to --out.

  python bench_sp.py --out profiles/sp_1M_20M.json
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

DELTAS = ("0.02", "0.1", "0.5", "2", "inf")


def weighted_ba(n, m):
    src, dst = ba_edges(n, m)
    w = 1.0 - np.random.default_rng(7).random(len(src))  # (0, 1]
    return src, dst, w


def pairs_of(n, n_starts, n_pairs, seed):
    rng = np.random.default_rng(seed)
    starts = np.repeat(rng.choice(np.arange(1000, n), n_starts, replace=False), n_pairs // n_starts)
    ends = np.where(np.arange(len(starts)) % 2 == 0, rng.integers(0, 1000, len(starts)), rng.integers(0, n, len(starts)))
    return starts.astype(np.int32), ends.astype(np.int32)


def check_against_model(pkg, n, m):
    import sp_model as sm

    src, dst, w = weighted_ba(n, m)
    g = pkg.graph.graph_from_edges(n, src, dst, w)
    out = sm.lists_of(n, src, dst, w)
    starts, ends = pairs_of(n, 4, 40, 1)
    row_off, node, dist = g.shortest_paths(starts, ends, mode="fast")
    found = 0
    for a in sorted(set(starts.tolist())):
        d = sm.distances(out, a)
        tree = sm.tight_levels(out, d, a)
        for i in np.flatnonzero(starts == a).tolist():
            nodes, dists = sm.canonical(out, a, int(ends[i]), d, tree)
            lo, hi = int(row_off[i]), int(row_off[i + 1])
            assert node[lo:hi].tolist() == nodes and dist[lo:hi].tolist() == dists, "bench_sp: fast rows differ from the model's"
            found += bool(nodes)
    g.close()
    return {"nodes": n, "edges": int(len(src)), "pairs": int(len(starts)), "found": found, "rows_equal_model": True}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=1_000_000)
    ap.add_argument("--attach", type=int, default=20, help="edges per arriving node (20 → 20M edges at 1M nodes)")
    ap.add_argument("--pairs", type=int, default=10_000)
    ap.add_argument("--starts", type=int, default=1_000)
    ap.add_argument("--loop-pairs", type=int, default=10_000, help="how many of the pairs are also sent one call each")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--check-nodes", type=int, default=100_000)
    ap.add_argument("--replay-nodes", type=int, default=10_000)
    ap.add_argument("--replay-rows", type=int, default=200_000)
    ap.add_argument("--replay-pairs", type=int, default=8)
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    import muninn_amd

    pkg = muninn_amd.pkg
    pkg.build()
    pkg.lib()
    assert pkg.device_count() >= 1, "bench_sp: no gfx950 device"
    med = statistics.median
    checked = check_against_model(pkg, args.check_nodes, args.attach)
    src, dst, w = weighted_ba(args.nodes, args.attach)
    g = pkg.graph.graph_from_edges(args.nodes, src, dst, w)
    starts, ends = pairs_of(args.nodes, args.starts, args.pairs, 2)

    def timed(fn):
        t0 = time.perf_counter()
        r = fn()
        return (time.perf_counter() - t0) * 1e3, r, dict(g.sp_stats)

    def one_pair():
        runs = [timed(lambda: g.shortest_paths(starts[:1], ends[:1], mode="fast")) for _ in range(args.runs)]
        st, wall = runs[0][2], med(r[0] for r in runs)
        return {"ms": wall, "device_ms": med(r[2]["device_ms"] for r in runs), "rows": int(len(runs[0][1][1])),
                "relaxations": st["relaxations"], "passes": st["passes"], "relaxations_per_s": st["relaxations"] / (wall * 1e-3)}

    def batch():
        runs = [timed(lambda: g.shortest_paths(starts, ends, mode="fast")) for _ in range(args.runs)]
        st, wall = runs[0][2], med(r[0] for r in runs)
        return runs[0][1], {"ms": wall, "device_ms": med(r[2]["device_ms"] for r in runs), "rows": int(len(runs[0][1][1])),
                            "found": int((np.diff(runs[0][1][0]) > 0).sum()), "chunks": st["chunks"], "sources": st["sources"],
                            "relaxations": st["relaxations"], "passes": st["passes"],
                            "relaxations_per_s": st["relaxations"] / (wall * 1e-3), "pairs_per_s": len(starts) / (wall * 1e-3)}

    os.environ.pop("MN_SSSP_DELTA", None)
    g.shortest_paths(starts[:1], ends[:1], mode="fast")  # warm-up: the weights' one scan
    single = one_pair()
    rows, many = batch()
    k = min(args.loop_pairs, len(starts))

    def singles():
        n_rows = 0
        for a, b in zip(starts[:k].tolist(), ends[:k].tolist()):
            n_rows += len(g.shortest_paths([a], [b], mode="fast")[1])
        return n_rows

    loop = [timed(singles) for _ in range(args.runs if k <= 1000 else 1)]
    assert loop[0][1] == int(rows[0][k]), "bench_sp: one call per pair gives other rows than one call for all"
    wall = med(r[0] for r in loop)
    many["as_single_calls"] = {"pairs": k, "ms": wall, "ms_per_call": wall / k, "pairs_per_s": k / (wall * 1e-3)}

    sweep = {}
    for delta in DELTAS:
        os.environ["MN_SSSP_DELTA"] = delta
        got, b = batch()
        assert all(np.array_equal(x.view(np.uint8), y.view(np.uint8)) for x, y in zip(rows, got)), "bench_sp: delta changed a row"
        sweep[delta] = {"one_pair": one_pair(), "batch": b}
    os.environ.pop("MN_SSSP_DELTA", None)
    g.close()

    # replay beside fast mode: at a tenth of the reference's published size and at that size; there also the compiled reference
    def replay_at(n, m, with_reference):
        rng = np.random.default_rng(3)
        rs, rd, rw = rng.integers(0, n, m), rng.integers(0, n, m), 1.0 - rng.random(m)
        g = pkg.graph.graph_from_edges(n, rs, rd, rw)
        ps, pe = rng.integers(0, n, args.replay_pairs).astype(np.int32), rng.integers(0, n, args.replay_pairs).astype(np.int32)

        def timed(fn):
            t0 = time.perf_counter()
            r = fn()
            return (time.perf_counter() - t0) * 1e3, r, dict(g.sp_stats)

        g.shortest_paths(ps[:1], pe[:1], mode="replay")
        rr = [timed(lambda: g.shortest_paths(ps, pe, mode="replay")) for _ in range(args.runs)]
        fr = [timed(lambda: g.shortest_paths(ps, pe, mode="fast")) for _ in range(args.runs)]
        one_r = [timed(lambda: g.shortest_paths(ps[:1], pe[:1], mode="replay")) for _ in range(args.runs)]
        one_f = [timed(lambda: g.shortest_paths(ps[:1], pe[:1], mode="fast")) for _ in range(args.runs)]
        (ro, _, rdist), (fo, _, fdist) = rr[0][1], fr[0][1]
        assert all((ro[i + 1] > ro[i]) == (fo[i + 1] > fo[i]) and (ro[i + 1] == ro[i] or rdist[ro[i + 1] - 1] == fdist[fo[i + 1] - 1])
                   for i in range(len(ps))), "bench_sp: replay and fast disagree on a distance"
        out = {"nodes": n, "rows": m, "pairs": int(len(ps)), "replay_ms": med(r[0] for r in rr), "fast_ms": med(r[0] for r in fr),
               "replay_device_ms": med(r[2]["device_ms"] for r in rr), "pops": rr[0][2]["pops"], "pushes": rr[0][2]["pushes"],
               "one_pair_replay_ms": med(r[0] for r in one_r), "one_pair_fast_ms": med(r[0] for r in one_f),
               "end_distances_equal_fast": True}
        g.close()
        ref_so = os.path.join(ROOT, "oracle", "_ref", "muninn.so")
        if with_reference and os.path.exists(ref_so):
            c = sqlite3.connect(":memory:")
            c.enable_load_extension(True)
            c.load_extension(ref_so[:-3])
            c.execute("CREATE TABLE e(s TEXT, d TEXT, w REAL)")
            c.executemany("INSERT INTO e VALUES (?, ?, ?)", zip(map(str, rs.tolist()), map(str, rd.tolist()), rw.tolist()))
            c.execute("CREATE INDEX e_s ON e(s)")  # (a node's rows still come in table order; without it every settle scans the table)
            t0 = time.perf_counter()
            ref_rows = [c.execute("SELECT node, distance FROM graph_shortest_path('e', 's', 'd', ?, ?, 'w')", (str(a), str(b))).fetchall()
                        for a, b in zip(ps.tolist(), pe.tolist())]
            out["reference_ms"] = (time.perf_counter() - t0) * 1e3
            row_off, node, dist = rr[0][1]
            ours = [[(str(v), x) for v, x in zip(node[a:b].tolist(), dist[a:b].tolist())] for a, b in zip(row_off[:-1], row_off[1:])]
            assert ours == ref_rows, "bench_sp: replay's rows differ from the compiled reference's"
            out["rows_equal_reference"] = True
            c.close()
        return out

    n, m = args.replay_nodes, args.replay_rows
    replay = {f"{n // k}x{m // k}": replay_at(n // k, m // k, k == 1) for k in (100, 50, 20, 10, 1)}
    res = {"workload": "graph_shortest_path", "graph": {"model": "barabasi-albert, forward lists, uniform (0, 1] weights",
                                                         "nodes": args.nodes, "edges": int(len(src))},
           "runs": args.runs, "one_pair_fast": single, "batch_fast": dict(many, pairs=int(len(starts)), starts=args.starts),
           "delta_sweep": sweep, "replay": replay, "checked_against_model": checked}
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
