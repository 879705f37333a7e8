#!/usr/bin/env python3
"""Exact (flat) search against the kernel it grew out of: mn_hnsw_search_exact_batch_dev (candidate pass on the f32 matrix cores,
re-score in the index's order, certificate; csrc/mn_exact.hip) and mn_hnsw_bruteforce_topk (k_brute_mfma, bench.py's ground
truth: ids only, ranked by the matrix cores' own arithmetic), timed on the same index and the same device buffers, in one
process, as interleaved pairs.  Also: how many queries failed their certificate, how many rows were re-scored, and recall@k of the
graph search (search_batch at --ef) against the exact answer — so that the trade between the two searches stands in one place.
The certificate counts are repeated on bench.py's clustered generator.

Prints ONE JSON line.

    python bench_exact.py [--n 1000000 --dim 768 --nq 10000 --k 10 --metric cosine --ef 128 --pairs 3]
"""
import argparse
import json
import sys
import time

import numpy as np

import bench
import muninn_amd


def progress(msg):
    print(f"[bench_exact {time.strftime('%H:%M:%S')}] {msg}", file=sys.stderr, flush=True)


class DevQueries:
    """queries and the exact search's outputs in device memory"""

    def __init__(self, g, Q, k):
        self.g, self.nq, self.k = g, len(Q), k
        self.q = g.dev_malloc(Q.nbytes)
        g.dev_upload(self.q, Q)
        self.ids, self.ds, self.cnt = g.dev_malloc(self.nq * k * 8), g.dev_malloc(self.nq * k * 4), g.dev_malloc(self.nq * 4)

    def exact(self):
        t0 = time.perf_counter()
        self.g.search_exact_batch_dev(self.q, self.nq, self.k, self.ids, self.ds, self.cnt)  # returns when its kernels are done
        return time.perf_counter() - t0

    def brute(self):
        t0 = time.perf_counter()
        out = self.g.bruteforce_topk(self.q, self.nq, self.k)
        return time.perf_counter() - t0, out

    def exact_ids(self):
        out = np.empty((self.nq, self.k), np.int64)
        self.g.dev_download(out, self.ids)
        return out

    def free(self):
        for p in (self.q, self.ids, self.ds, self.cnt):
            self.g.dev_free(p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--nq", type=int, default=10_000)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--metric", default="cosine")
    ap.add_argument("--ef", type=int, default=128)
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--clustered", default="clustered", help="bench.py dataset the certificate counts are repeated on ('' = skip)")
    args = ap.parse_args()
    pkg = muninn_amd.pkg
    pkg.lib()
    if pkg.device_count() < 1:
        raise SystemExit("bench_exact.py: no gfx950 device")
    N, D, NQ, K = args.n, args.dim, args.nq, args.k

    progress(f"generating {N} x {D} gaussian")
    X = bench.gen_vectors(N, D, 42, "gaussian")
    Q = bench.gen_vectors(NQ, D, 43, "gaussian")
    g = pkg.HnswIndex(D, args.metric, 16, 200)
    t0 = time.perf_counter()
    if g.build(np.arange(1, N + 1, dtype=np.int64), X, 16, 8192) != 0:
        raise SystemExit("bench_exact.py: build failed")
    g.sync()
    build_s = time.perf_counter() - t0
    del X
    progress(f"built in {build_s:.1f}s")
    dq = DevQueries(g, Q, K)
    dq.exact()  # warm-up of both
    dq.brute()
    pairs = []
    for _ in range(args.pairs):
        te = dq.exact()
        st = g.last_exact()
        tb, truth = dq.brute()
        pairs.append({"exact_ms": te * 1e3, "exact_kernel_ms": st["kernel_ms"], "bruteforce_ms": tb * 1e3,
                      "bruteforce_kernel_ms": g.last_launch()["last_kernel_ms"], "ratio": te / tb})
        progress(f"pair: exact {te * 1e3:.1f} ms, bruteforce_topk {tb * 1e3:.1f} ms")
    exact_ids = dq.exact_ids()
    # the graph search at --ef against the exact answer
    d_i, d_d, d_c = g.dev_malloc(NQ * K * 8), g.dev_malloc(NQ * K * 4), g.dev_malloc(NQ * 4)
    g.search_batch_dev(dq.q, NQ, K, args.ef, d_i, d_d, d_c)
    g.sync()
    hn = np.empty((NQ, K), np.int64)
    g.dev_download(hn, d_i)
    for p in (d_i, d_d, d_c):
        g.dev_free(p)
    e_ms = float(np.median([p["exact_ms"] for p in pairs]))
    b_ms = float(np.median([p["bruteforce_ms"] for p in pairs]))
    out = {
        "config": {"n": N, "dim": D, "nq": NQ, "k": K, "metric": args.metric, "order": "sse", "dataset": "gaussian",
                   "M": 16, "ef_construction": 200},
        "pairs": pairs,
        "exact_ms": e_ms, "bruteforce_topk_ms": b_ms, "ratio": e_ms / b_ms,
        "exact_queries_per_s": NQ / (e_ms * 1e-3),
        "exact_tflops": 2.0 * N * D * NQ / (e_ms * 1e-3) / 1e12,
        "n_mfma_queries": st["n_mfma_queries"], "n_fallback_queries": st["n_fallback_queries"],
        "n_rescored_rows": st["n_rescored_rows"], "n_bound_violations": st["n_bound_violations"],
        # k_brute_mfma ranks by its own arithmetic: near-equal distances may swap places against the index's order
        "ids_equal_to_bruteforce_topk": float(np.mean(exact_ids == truth)),
        "set_recall_of_bruteforce_topk_vs_exact": bench.recall_of(truth, exact_ids, K),
        "hnsw": {"ef": args.ef, f"recall_at_{K}_vs_exact": bench.recall_of(hn, exact_ids, K)},
        "build_s": build_s,
    }
    dq.free()
    g.close()

    if args.clustered:
        progress(f"generating {N} x {D} {args.clustered}")
        X = bench.gen_vectors(N, D, 42, args.clustered)
        Qc = bench.gen_vectors(NQ, D, 43, args.clustered)
        # the exact search reads no link: a thin graph is enough to put the rows on the device
        g = pkg.HnswIndex(D, args.metric, 4, 8)
        if g.build(np.arange(1, N + 1, dtype=np.int64), X, 16, 8192) != 0:
            raise SystemExit("bench_exact.py: build failed")
        g.sync()
        del X
        dq = DevQueries(g, Qc, K)
        dq.exact()
        te = dq.exact()
        st = g.last_exact()
        out["clustered"] = {"dataset": args.clustered, "what": bench.dataset_note(args.clustered, D), "exact_ms": te * 1e3,
                            "exact_kernel_ms": st["kernel_ms"], "n_fallback_queries": st["n_fallback_queries"],
                            "n_rescored_rows": st["n_rescored_rows"], "n_bound_violations": st["n_bound_violations"]}
        dq.free()
        g.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
