// mn_graph_int.hpp — what the translation units behind the mn_graph handle share: mn_graph.hip (handle, CSR upload),
// mn_csr_build.hip (the handle built on the device from an edge list),
// mn_leiden.hip (with mn_leiden_eval.hpp, the device code of its evaluation, included by it alone), mn_centrality.hip and
// mn_bfs.hip, mn_dfs.hip, mn_select.hip and mn_sssp.hip.  Host declarations and the kernels' view of the CSR only: device code does not cross a translation unit, every
// kernel lives in the file that launches it.
#pragma once
#include "../../include/muninn_hip.h"
#include "mn_host.hpp"

#include <algorithm>
#include <atomic>
#include <cstdlib>

#define DEVI __device__ __forceinline__

struct DevGraph {
    int n;
    const int *off_out, *tgt_out;
    const double *w_out; // null = 1.0
    const int *off_in, *tgt_in;
    const double *w_in;
};

struct LeiWork; // mn_leiden.hip
struct BfsWork; // mn_bfs.hip
struct DfsWork; // mn_dfs.hip
struct SelWork; // mn_select.hip
struct SpWork;  // mn_sssp.hip

struct mn_graph {
    std::atomic<int> refs{1}; // owners: mn_graph_retain adds one, mn_graph_destroy releases one and the last frees
    int device = 0;
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    int n = 0;
    long long e_out = 0, e_in = 0;
    int max_deg_both = 0, max_deg_out = 0;
    bool weighted = false;
    int *off_out = nullptr, *tgt_out = nullptr, *off_in = nullptr, *tgt_in = nullptr;
    double *w_out = nullptr, *w_in = nullptr;
    double last_ms = 0;
    mn_leiden_stats stats = {};
    std::vector<int> h_off_out, h_off_in; // host copies of the offsets (degrees: list of wide nodes, scratch sizing)
    struct LeiWork *work = nullptr;       // run_leiden's device buffers, allocated on first use and kept
    struct BfsWork *bfs = nullptr;        // mn_graph_bfs's scratch and the rows of its last call, likewise
    struct DfsWork *dfs = nullptr;        // mn_graph_dfs's, likewise
    struct SelWork *sel = nullptr;        // mn_graph_select's, likewise
    struct SpWork *sp = nullptr;          // mn_graph_shortest_paths's weight summary and the rows of its last call
};

inline DevGraph dev_graph_of(const mn_graph *g) { return {g->n, g->off_out, g->tgt_out, g->w_out, g->off_in, g->tgt_in, g->w_in}; }

// the thread's mn_graph_last_error string (mn_graph.hip)
void gset_err(const char *fmt, ...) __attribute__((format(printf, 1, 2)));
#define GCHK(expr) MN_HIPCHK(gset_err, expr)

// device time between the handle's two events → mn_graph_last_ms
inline void graph_note_ms(mn_graph *g) {
    float ms = 0;
    if (hipEventElapsedTime(&ms, g->ev0, g->ev1) == hipSuccess)
        g->last_ms = ms;
}

// Scratch a call may take: half of what the device has free once `reserve` bytes are set aside, at least 256 MiB — unless
// the environment variable `env` gives a decimal number of MiB (fractions allowed, <= 0 means 0).
inline size_t scratch_budget(const char *env, size_t reserve) {
    size_t budget = (size_t)8 << 30, free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) == hipSuccess)
        budget = std::max<size_t>((size_t)256 << 20, (free_b > reserve ? free_b - reserve : 0) / 2);
    if (const char *e = getenv(env)) {
        const double mb = strtod(e, nullptr);
        budget = mb > 0 ? (size_t)(mb * 1048576.0) : 0;
    }
    return budget;
}

void lei_work_free(LeiWork *w); // mn_leiden.hip: releases and deletes a graph's Leiden workspace (mn_graph_destroy)
void bfs_work_free(BfsWork *w); // mn_bfs.hip: the same for the traversal's
void dfs_work_free(DfsWork *w); // mn_dfs.hip: the same for the depth-first traversal's
void sel_work_free(SelWork *w); // mn_select.hip: the same for the selectors'
void sp_work_free(SpWork *w);   // mn_sssp.hip: the same for the shortest paths'
