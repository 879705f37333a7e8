#!/usr/bin/env python3
"""Entity resolution's device stages on one index: mn_hnsw_er_edges (blocking, candidate pairs, scoring cascade) with both
blockings — the reference's graph search at k + 1 and the exact k-NN graph — on synthetic records: groups of near-duplicate
vectors whose names are edited copies of one another.

Reported per blocking: wall time of the whole call (names up, edges down), device time per stage (HIP events), candidates,
edges, how many pairs ran the Jaro-Winkler loop one per lane and one per wavefront, and pairs per second of the scoring stage;
and, as "staged", the wall time of each stage when a host runs them one by one through the host-array entry points (the search
or knn_graph, then er.candidates, then er.score: every list crosses the host link twice) — the edges of the two ways must agree
on every bit before anything is reported.
No ratio is claimed: nothing older computes this on the device, and the reference is a CPU program that is not run here.
The line is printed and written to --out.

    python bench_er.py [--rows 200000 --dim 768 --k 10 --group 4 --repeats 3 --out profiles/er_200kx768.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

import muninn_amd

ROOT = os.path.dirname(os.path.abspath(__file__))


def progress(msg):
    print(f"[bench_er {time.strftime('%H:%M:%S')}] {msg}", file=sys.stderr, flush=True)


def records(n, dim, group, seed):
    """n vectors in groups of `group` around a gaussian centre (noise 0.15 sigma per coordinate: cosine distance ~0.02 inside a
    group, ~1 across), and one name per row: a random 8-40 byte stem per group, each member an edited copy (case, a swapped
    pair of bytes, a dropped byte, a suffix) or the stem itself."""
    rng = np.random.default_rng(seed)
    n_groups = (n + group - 1) // group
    centres = rng.standard_normal((n_groups, dim), dtype=np.float32)
    gid = np.arange(n) // group
    X = centres[gid]
    X += 0.15 * rng.standard_normal((n, dim), dtype=np.float32)
    letters = np.frombuffer(b"abcdefghijklmnopqrstuvwxyz ABCDEFGHIJKLMNOP", np.uint8)
    lens = rng.integers(8, 41, n_groups)
    stems = [bytes(letters[rng.integers(0, len(letters), int(l))]) for l in lens]
    how = rng.integers(0, 6, n)
    at = rng.random(n)
    names = []
    for i in range(n):
        s = stems[gid[i]]
        p = int(at[i] * (len(s) - 1))
        if how[i] == 1:
            s = s.upper()
        elif how[i] == 2:
            s = s[:p] + s[p + 1:p + 2] + s[p:p + 1] + s[p + 2:]
        elif how[i] == 3:
            s = s[:p] + s[p + 1:]
        elif how[i] == 4:
            s = s + b" Inc"
        names.append(s)
    sources = [(b"a", b"b", b"c")[i % 3] for i in range(n)]
    return X, names, sources


def staged(pkg, g, ids, names, sources, k, thr, jw_weight, blocking):
    """the same edges from the stages run one by one with host arrays in between: (edges, wall ms per stage)"""
    t0 = time.perf_counter()
    if blocking == "graph":
        Q = g.export_vectors()  # every row is live and in id order here: the stored vectors are the queries
        t1 = time.perf_counter()
        ni, nd, nc = g.search_batch(Q, k + 1, 2 * (k + 1))
        wall = {"export_ms": (t1 - t0) * 1e3, "blocking_ms": (time.perf_counter() - t1) * 1e3}
    else:
        cut = np.float32(thr)
        if float(cut) > thr:
            cut = np.nextafter(cut, np.float32(-1))
        ni, nd, nc = g.knn_graph_slots(k, cut)
        wall = {"blocking_ms": (time.perf_counter() - t0) * 1e3}
    t2 = time.perf_counter()
    r1, r2, d = pkg.er.candidates(ids, ni, nd, nc, thr)
    t3 = time.perf_counter()
    edges = pkg.er.score(r1, r2, d, names, sources, "same_source", jw_weight, 1.0 - thr)
    t4 = time.perf_counter()
    wall.update(candidates_ms=(t3 - t2) * 1e3, score_ms=(t4 - t3) * 1e3, total_ms=(t4 - t0) * 1e3)
    return edges, wall


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=200_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--group", type=int, default=4)
    ap.add_argument("--M", type=int, default=16)
    ap.add_argument("--efc", type=int, default=100)
    ap.add_argument("--dist-threshold", type=float, default=0.15)
    ap.add_argument("--jw-weight", type=float, default=0.3)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None, help="where the line is written (default profiles/er_<rows/1000>kx<dim>.json)")
    args = ap.parse_args()
    pkg = muninn_amd.pkg
    pkg.lib()
    if pkg.device_count() < 1:
        raise SystemExit("bench_er.py: no gfx950 device")
    N, D, K = args.rows, args.dim, args.k
    out_path = args.out or os.path.join(ROOT, "profiles", f"er_{N // 1000}kx{D}.json")

    progress(f"generating {N} x {D} in groups of {args.group}")
    X, names, sources = records(N, D, args.group, 42)
    ids = np.arange(1, N + 1, dtype=np.int64)
    g = pkg.HnswIndex(D, "cosine", args.M, args.efc)
    t0 = time.perf_counter()
    if g.build(ids, X, 16, 8192) != 0:
        raise SystemExit("bench_er.py: build failed")
    g.sync()
    build_s = time.perf_counter() - t0
    del X
    progress(f"index built in {build_s:.1f}s")

    out = {"config": {"rows": N, "dim": D, "k": K, "group": args.group, "metric": "cosine", "M": args.M, "ef_construction": args.efc,
                      "dist_threshold": args.dist_threshold, "jw_weight": args.jw_weight, "type_guard": "same_source",
                      "name_bytes": int(sum(len(s) for s in names)), "repeats": args.repeats},
           "build_s": build_s}
    for blocking in ("graph", "exact"):
        runs = []
        for r in range(args.repeats + 1):  # the first run is the warm-up
            t0 = time.perf_counter()
            edges, st = pkg.er.resolve(g, ids, names, sources, K, args.dist_threshold, args.jw_weight, 0.0, "same_source", blocking,
                                       return_stats=True)
            st["wall_ms"] = (time.perf_counter() - t0) * 1e3
            if r:
                runs.append(st)
            progress(f"{blocking}: wall {st['wall_ms']:.1f} ms, blocking {st['blocking_ms']:.1f} candidates {st['candidates_ms']:.2f} "
                     f"score {st['score_ms']:.2f} ms on the device; {st['n_candidates']} candidates, {st['n_edges']} edges")
        med = {key: float(np.median([x[key] for x in runs])) for key in ("wall_ms", "blocking_ms", "candidates_ms", "score_ms")}
        walls = []
        for r in range(args.repeats):
            e2, w = staged(pkg, g, ids, names, sources, K, args.dist_threshold, args.jw_weight, blocking)
            if e2.tobytes() != edges.tobytes():
                raise SystemExit(f"bench_er.py: {blocking}: the stages run one by one and mn_hnsw_er_edges disagree")
            walls.append(w)
            progress(f"{blocking} staged: " + ", ".join(f"{key} {v:.1f}" for key, v in w.items()))
        med["staged_wall_ms"] = {key: float(np.median([w[key] for w in walls])) for key in walls[0]}
        last = runs[-1]
        same_group = int(np.sum((edges["r1"] // args.group) == (edges["r2"] // args.group)))
        out[blocking] = dict(med, n_candidates=last["n_candidates"], n_edges=last["n_edges"], n_jw_short=last["n_jw_short"],
                             n_jw_long=last["n_jw_long"], edges_inside_a_group=same_group,
                             score_pairs_per_s=last["n_candidates"] / (med["score_ms"] * 1e-3) if med["score_ms"] > 0 else None,
                             candidate_entries_per_s=N * (K + (blocking == "graph")) / (med["candidates_ms"] * 1e-3)
                             if med["candidates_ms"] > 0 else None,
                             runs=runs)
    g.close()
    line = json.dumps(out)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
