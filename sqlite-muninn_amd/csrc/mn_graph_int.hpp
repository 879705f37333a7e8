// mn_graph_int.hpp — what the translation units behind the mn_graph handle share:
//   mn_graph.hip        the handle and the CSR upload
//   mn_csr_build.hip    the handle built on the device from an edge list
//   mn_leiden.hip       with mn_leiden_eval.hpp, the device code of its evaluation, which it alone includes
//   mn_centrality.hip   betweenness, closeness, degree
//   mn_bfs.hip, mn_dfs.hip (with mn_traverse.hpp: a seed traversal's argument checks and row store), mn_select.hip,
//   mn_sssp.hip         the entry points that keep scratch and the rows of their last call with the handle
// Here: the handle, the kernels' view of the CSR, the error string, and the host idioms every such entry point repeats —
// the direction argument, device time between the handle's two events, the scratch budget and the chunk it admits, the
// clamped grid size.  mn_host.hpp has the owned device array (DevBuf), mn_prim.hpp rocPRIM's two-phase call.  Host
// declarations only: device code does not cross a translation unit, every kernel lives in the file that launches it.
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

// direction 0 (both), 1 (forward) or 2 (reverse) → the lists a traversal follows; anything else is `who`'s error
inline int graph_direction(const char *who, int direction, int *use_out, int *use_in) {
    if (direction < 0 || direction > 2) {
        gset_err("%s: direction must be 0 (both), 1 (forward) or 2 (reverse)", who);
        return -1;
    }
    *use_out = direction != 2;
    *use_in = direction != 1;
    return 0;
}

// Device time is what lies between the handle's two events.  The caller records ev0 where its launches begin;
// graph_mark records ev1 behind them and picks up a launch error; graph_wait waits for the stream and adds ev0 .. ev1 to
// *ms.  A read-back queued between the two rides on the same wait.
inline int graph_mark(mn_graph *g) {
    GCHK(hipEventRecord(g->ev1, g->stream));
    GCHK(hipGetLastError());
    return 0;
}
inline int graph_wait(mn_graph *g, double *ms) {
    GCHK(hipStreamSynchronize(g->stream));
    float t = 0;
    if (hipEventElapsedTime(&t, g->ev0, g->ev1) == hipSuccess)
        *ms += t;
    return 0;
}
inline int graph_mark_wait(mn_graph *g, double *ms) { return graph_mark(g) || graph_wait(g, ms) ? -1 : 0; }

// the same interval → mn_graph_last_ms, for a call that has waited already
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
// how many of `n` items go through at once at `per_item` bytes of scratch each: at least one, at most `cap`
inline size_t scratch_chunk(size_t n, size_t budget, size_t per_item, size_t cap) {
    return std::max<size_t>(1, std::min({n, budget / per_item, cap}));
}

// workgroups for `items` at `per_block` each: at least one, at most `max_blocks`
inline unsigned launch_blocks(unsigned long long items, unsigned per_block, unsigned max_blocks) {
    return (unsigned)std::max<unsigned long long>(1, std::min<unsigned long long>((items + per_block - 1) / per_block, max_blocks));
}

void lei_work_free(LeiWork *w); // mn_leiden.hip: releases and deletes a graph's Leiden workspace (mn_graph_destroy)
void bfs_work_free(BfsWork *w); // mn_bfs.hip: the same for the traversal's
void dfs_work_free(DfsWork *w); // mn_dfs.hip: the same for the depth-first traversal's
void sel_work_free(SelWork *w); // mn_select.hip: the same for the selectors'
void sp_work_free(SpWork *w);   // mn_sssp.hip: the same for the shortest paths'
