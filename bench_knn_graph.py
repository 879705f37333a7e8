#!/usr/bin/env python3
"""The exact k-NN graph of an index's own rows, two ways on one index in one process, as interleaved pairs:

  (a) HnswIndex.knn_graph_slots — mn_hnsw_knn_graph: the self-join on the device, no vector leaving HBM (csrc/mn_exact.hip,
      DESIGN.md §3.7);
  (b) the only way without it: export_vectors, then search_exact_batch with those rows as queries at k + 1 in batches of 16384,
      then dropping each row's own id on the host (the same answer under the (d, slot) rule).

(a) and (b) must agree on every id and every distance bit before anything is reported.  Reported: time per call of both, how much
of (b) is host transfer (everything but its kernels: the export, the query upload, the result download), TFLOP/s, the
last_exact counters, edges per second and the ratio (a)/(b).  The line is printed and written to --out.

    python bench_knn_graph.py [--rows 200000 --dim 768 --k 10 --metric cosine --pairs 3 --out profiles/knn_graph_200kx768.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

import bench
import muninn_amd

ROOT = os.path.dirname(os.path.abspath(__file__))
QUERY_BATCH = 16384


def progress(msg):
    print(f"[bench_knn_graph {time.strftime('%H:%M:%S')}] {msg}", file=sys.stderr, flush=True)


def self_join(g, k):
    """(a): (ids, dists, counts) by slot, wall seconds, last_exact"""
    t0 = time.perf_counter()
    out = g.knn_graph_slots(k)
    return out, time.perf_counter() - t0, g.last_exact()


def host_loop(g, ids, k):
    """(b): the same arrays through export_vectors + search_exact_batch at k + 1 + a host pass; wall seconds split by step"""
    n = len(ids)
    t0 = time.perf_counter()
    X = g.export_vectors()
    t_export = time.perf_counter() - t0
    ni = np.empty((n, k + 1), np.int64)
    nd = np.empty((n, k + 1), np.float32)
    nc = np.empty(n, np.int32)
    kernel_ms, t_search, fallback, rescored = 0.0, 0.0, 0, 0
    for s in range(0, n, QUERY_BATCH):
        t1 = time.perf_counter()
        ni[s:s + QUERY_BATCH], nd[s:s + QUERY_BATCH], nc[s:s + QUERY_BATCH] = g.search_exact_batch(X[s:s + QUERY_BATCH], k + 1)
        t_search += time.perf_counter() - t1
        st = g.last_exact()
        kernel_ms += st["kernel_ms"]
        fallback += st["n_fallback_queries"]
        rescored += st["n_rescored_rows"]
    t2 = time.perf_counter()
    # drop the row's own id (where k + 1 duplicates in lower slots push it out of the list, the last entry goes instead)
    drop = ni == ids[:, None]
    drop[~drop.any(axis=1), k] = True
    first = np.argmax(drop, axis=1)
    cols = np.arange(k)[None, :] + (np.arange(k)[None, :] >= first[:, None])
    oi, od = np.take_along_axis(ni, cols, axis=1), np.take_along_axis(nd, cols, axis=1)
    oc = np.minimum(nc - (first < nc), k).astype(np.int32)
    t_drop = time.perf_counter() - t2
    total = time.perf_counter() - t0
    return (oi, od, oc), {"total_ms": total * 1e3, "export_ms": t_export * 1e3, "search_ms": t_search * 1e3,
                          "kernel_ms": kernel_ms, "drop_self_ms": t_drop * 1e3, "n_fallback_queries": fallback,
                          "n_rescored_rows": rescored}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=200_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--metric", default="cosine")
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--out", default=None, help="where the line is written (default profiles/knn_graph_<rows/1000>kx<dim>.json)")
    args = ap.parse_args()
    pkg = muninn_amd.pkg
    pkg.lib()
    if pkg.device_count() < 1:
        raise SystemExit("bench_knn_graph.py: no gfx950 device")
    N, D, K = args.rows, args.dim, args.k
    out_path = args.out or os.path.join(ROOT, "profiles", f"knn_graph_{N // 1000}kx{D}.json")

    progress(f"generating {N} x {D} gaussian")
    X = bench.gen_vectors(N, D, 42, "gaussian")
    ids = np.arange(1, N + 1, dtype=np.int64)
    g = pkg.HnswIndex(D, args.metric, 4, 8)  # neither way reads a link: a thin graph is enough to put the rows on the device
    t0 = time.perf_counter()
    if g.build(ids, X, 16, 8192) != 0:
        raise SystemExit("bench_knn_graph.py: build failed")
    g.sync()
    build_s = time.perf_counter() - t0
    del X
    progress(f"built in {build_s:.1f}s")

    a_out, _, _ = self_join(g, K)  # warm-up of both, and the agreement that everything below rests on
    b_out, _ = host_loop(g, ids, K)
    same = (np.array_equal(a_out[0], b_out[0]) and np.array_equal(a_out[1].view(np.int32), b_out[1].view(np.int32))
            and np.array_equal(a_out[2], b_out[2]))
    if not same:
        raise SystemExit("bench_knn_graph.py: knn_graph and the search_exact_batch loop disagree")
    progress("knn_graph == export_vectors + search_exact_batch(k + 1) - self, every id and distance bit")
    pairs = []
    for _ in range(args.pairs):
        _, ta, st = self_join(g, K)
        _, tb = host_loop(g, ids, K)
        pairs.append({"knn_graph_ms": ta * 1e3, "knn_graph_kernel_ms": st["kernel_ms"], "host_loop": tb,
                      "ratio": ta * 1e3 / tb["total_ms"]})
        progress(f"pair: knn_graph {ta * 1e3:.1f} ms, host loop {tb['total_ms']:.1f} ms (kernels {tb['kernel_ms']:.1f} ms)")
    a_ms = float(np.median([p["knn_graph_ms"] for p in pairs]))
    b_all = [p["host_loop"]["total_ms"] for p in pairs]
    b_ms = float(np.median(b_all))
    b_kernel = float(np.median([p["host_loop"]["kernel_ms"] for p in pairs]))
    edges = int(a_out[2].sum())
    flop = 2.0 * N * N * D
    out = {
        "config": {"rows": N, "dim": D, "k": K, "metric": args.metric, "order": "sse", "dataset": "gaussian",
                   "query_batch": QUERY_BATCH},
        "pairs": pairs,
        "knn_graph_ms": a_ms, "knn_graph_kernel_ms": float(np.median([p["knn_graph_kernel_ms"] for p in pairs])),
        "host_loop_ms": b_ms, "host_loop_ms_min_max": [min(b_all), max(b_all)], "host_loop_kernel_ms": b_kernel,
        "host_loop_transfer_share": 1.0 - b_kernel / b_ms,  # everything of (b) that is not its kernels
        "ratio": a_ms / b_ms,
        "knn_graph_tflops": flop / (a_ms * 1e-3) / 1e12, "host_loop_tflops": flop / (b_ms * 1e-3) / 1e12,
        "edges": edges, "edges_per_s": edges / (a_ms * 1e-3),
        "n_queries": st["n_queries"], "n_mfma_queries": st["n_mfma_queries"], "n_fallback_queries": st["n_fallback_queries"],
        "n_rescored_rows": st["n_rescored_rows"], "n_bound_violations": st["n_bound_violations"],
        "answers_equal": True, "build_s": build_s,
    }
    g.close()
    line = json.dumps(out)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
