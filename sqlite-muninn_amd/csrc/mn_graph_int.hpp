// mn_graph_int.hpp — what the translation units behind the mn_graph handle share: mn_graph.hip (handle, CSR upload),
// mn_leiden.hip and mn_centrality.hip.  Host declarations and the kernels' view of the CSR only: device code does not
// cross a translation unit, every kernel lives in the file that launches it.
#pragma once
#include "../../include/muninn_hip.h"
#include "mn_host.hpp"

#define DEVI __device__ __forceinline__

struct DevGraph {
    int n;
    const int *off_out, *tgt_out;
    const double *w_out; // null = 1.0
    const int *off_in, *tgt_in;
    const double *w_in;
};

struct LeiWork; // mn_leiden.hip

struct mn_graph {
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

void lei_work_free(LeiWork *w); // mn_leiden.hip: releases and deletes a graph's Leiden workspace (mn_graph_destroy)
