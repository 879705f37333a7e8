// mn_graph.hip — the mn_graph handle: device-resident CSR adjacency (src/graph_csr.h:27-34) uploaded once and shared by
// the algorithms over it (mn_leiden.hip + mn_leiden_eval.hpp, mn_centrality.hip, mn_bfs.hip, mn_dfs.hip, mn_select.hip, mn_sssp.hip), and their common error string.
// Host code only.
#include "mn_graph_int.hpp"
#include "mn_guard.hpp"

#include <algorithm>
#include <cstring>

static thread_local std::string g_gerr;
void gset_err(const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    mn_vformat(g_gerr, fmt, ap);
    va_end(ap);
}
extern "C" const char *mn_graph_last_error(void) { return g_gerr.c_str(); }

template <typename T> static int up(T **dst, const T *src, size_t n) {
    *dst = nullptr;
    GCHK(hipMalloc(dst, (n ? n : 1) * sizeof(T)));
    if (n)
        GCHK(hipMemcpy(*dst, src, n * sizeof(T), hipMemcpyHostToDevice));
    return 0;
}

extern "C" mn_graph *mn_graph_create(int n_nodes, const int *off_out, const int *tgt_out, const double *w_out,
                                     const int *off_in, const int *tgt_in, const double *w_in, int device) try {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) {
        gset_err("mn_graph_create: HIP device %d not available (no CPU fallback)", device);
        return nullptr;
    }
    if (n_nodes < 0 || !off_out || !off_in) {
        gset_err("mn_graph_create: bad arguments");
        return nullptr;
    }
    mn_graph *g = new mn_graph();
    g->device = device;
    g->n = n_nodes;
    g->e_out = n_nodes ? off_out[n_nodes] : 0;
    g->e_in = n_nodes ? off_in[n_nodes] : 0;
    g->weighted = w_out != nullptr || w_in != nullptr;
    for (int v = 0; v < n_nodes; v++) {
        int dO = off_out[v + 1] - off_out[v], dI = off_in[v + 1] - off_in[v];
        if (dO > g->max_deg_out) g->max_deg_out = dO;
        if (dO + dI > g->max_deg_both) g->max_deg_both = dO + dI;
    }
    bool ok = hipSetDevice(device) == hipSuccess && hipStreamCreateWithFlags(&g->stream, hipStreamNonBlocking) == hipSuccess &&
              hipEventCreate(&g->ev0) == hipSuccess && hipEventCreate(&g->ev1) == hipSuccess;
    ok = ok && up(&g->off_out, off_out, (size_t)n_nodes + 1) == 0 && up(&g->tgt_out, tgt_out, (size_t)g->e_out) == 0 &&
         up(&g->off_in, off_in, (size_t)n_nodes + 1) == 0 && up(&g->tgt_in, tgt_in, (size_t)g->e_in) == 0;
    if (ok && w_out)
        ok = up(&g->w_out, w_out, (size_t)g->e_out) == 0;
    if (ok && w_in)
        ok = up(&g->w_in, w_in, (size_t)g->e_in) == 0;
    if (!ok) {
        mn_graph_destroy(g);
        return nullptr;
    }
    g->h_off_out.assign(off_out, off_out + n_nodes + 1);
    g->h_off_in.assign(off_in, off_in + n_nodes + 1);
    return g;
} MN_GUARD_END(gset_err, MN_NOTHING, nullptr)

// One direction of a blocked CSR (the rows of "{t}_csr_fwd" / "{t}_csr_rev") straight into device buffers: per
// block, node count = offsets_bytes/4 - 1 and edge count = targets_bytes/4 (csr_deserialize, src/graph_csr.c:122-163);
// offsets are rebased by the running edge count, targets are already global (csr_merge_blocks, :402-477).
static int upload_blocks(const mn_csr_block *blk, int nb, int n_nodes, std::vector<int> &off, int **d_tgt, double **d_w,
                         long long *n_edges, bool *weighted) {
    off.assign((size_t)n_nodes + 1, 0);
    long long edges = 0;
    for (int b = 0; b < nb; b++) {
        if (!blk[b].offsets || blk[b].offsets_bytes < 4 || blk[b].targets_bytes < 0 || blk[b].targets_bytes % 4) {
            gset_err("mn_graph_create_blocked: block %d is malformed", b);
            return -1;
        }
        edges += blk[b].targets_bytes / 4;
    }
    if (edges > 0x7fffffffLL) {
        gset_err("mn_graph_create_blocked: %lld edges exceed int32 offsets", edges);
        return -1;
    }
    *weighted = nb > 0 && blk[0].weights != nullptr && blk[0].weights_bytes > 0; // has_weights of the first block (:415)
    *d_tgt = nullptr;
    *d_w = nullptr;
    GCHK(hipMalloc(d_tgt, (size_t)std::max<long long>(1, edges) * sizeof(int)));
    if (*weighted)
        GCHK(hipMalloc(d_w, (size_t)std::max<long long>(1, edges) * sizeof(double)));
    long long eoff = 0;
    int noff = 0;
    for (int b = 0; b < nb; b++) {
        const int bn = blk[b].offsets_bytes / 4 - 1, be = blk[b].targets_bytes / 4;
        const int *bo = static_cast<const int *>(blk[b].offsets);
        for (int i = 0; i < bn && noff + i < n_nodes; i++) {
            if (bo[i] < 0 || bo[i] > be) {
                gset_err("mn_graph_create_blocked: block %d offsets out of range", b);
                return -1;
            }
            off[(size_t)noff + i] = (int)(bo[i] + eoff);
        }
        if (be > 0 && blk[b].targets)
            GCHK(hipMemcpy(*d_tgt + eoff, blk[b].targets, (size_t)be * sizeof(int), hipMemcpyHostToDevice));
        if (*weighted && be > 0) {
            if (!blk[b].weights || blk[b].weights_bytes != be * 8) {
                gset_err("mn_graph_create_blocked: block %d weights do not match its targets", b);
                return -1;
            }
            GCHK(hipMemcpy(*d_w + eoff, blk[b].weights, (size_t)be * sizeof(double), hipMemcpyHostToDevice));
        }
        eoff += be;
        noff += bn;
    }
    for (int i = std::min(noff, n_nodes); i <= n_nodes; i++) // sentinel, and nodes the blocks did not cover (:470-475)
        off[(size_t)i] = (int)eoff;
    *n_edges = eoff;
    return 0;
}

extern "C" mn_graph *mn_graph_create_blocked(int n_nodes, const mn_csr_block *fwd, int n_fwd, const mn_csr_block *rev, int n_rev,
                                             int device) try {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) {
        gset_err("mn_graph_create_blocked: HIP device %d not available (no CPU fallback)", device);
        return nullptr;
    }
    if (n_nodes < 0 || n_fwd < 0 || n_rev < 0 || (n_fwd && !fwd) || (n_rev && !rev)) {
        gset_err("mn_graph_create_blocked: bad arguments");
        return nullptr;
    }
    mn_graph *g = new mn_graph();
    g->device = device;
    g->n = n_nodes;
    std::vector<int> oo, oi;
    bool wo = false, wi = false;
    bool ok = hipSetDevice(device) == hipSuccess && hipStreamCreateWithFlags(&g->stream, hipStreamNonBlocking) == hipSuccess &&
              hipEventCreate(&g->ev0) == hipSuccess && hipEventCreate(&g->ev1) == hipSuccess;
    ok = ok && upload_blocks(fwd, n_fwd, n_nodes, oo, &g->tgt_out, &g->w_out, &g->e_out, &wo) == 0 &&
         upload_blocks(rev, n_rev, n_nodes, oi, &g->tgt_in, &g->w_in, &g->e_in, &wi) == 0;
    if (ok) {
        // out-of-range targets would fault in the kernels: the rows come from a file, so look before launching
        std::vector<int> chk;
        for (int dir = 0; dir < 2 && ok; dir++) {
            const long long ne = dir ? g->e_in : g->e_out;
            chk.resize((size_t)ne);
            if (ne)
                ok = hipMemcpy(chk.data(), dir ? g->tgt_in : g->tgt_out, (size_t)ne * sizeof(int), hipMemcpyDeviceToHost) == hipSuccess;
            for (long long e = 0; e < ne && ok; e++)
                if (chk[(size_t)e] < 0 || chk[(size_t)e] >= n_nodes) {
                    gset_err("mn_graph_create_blocked: target %d out of range", chk[(size_t)e]);
                    ok = false;
                }
        }
    }
    if (ok) {
        g->weighted = wo || wi;
        for (int v = 0; v < n_nodes; v++) {
            int dO = oo[v + 1] - oo[v], dI = oi[v + 1] - oi[v];
            if (dO < 0 || dI < 0) {
                gset_err("mn_graph_create_blocked: offsets are not monotone at node %d", v);
                ok = false;
                break;
            }
            if (dO > g->max_deg_out) g->max_deg_out = dO;
            if (dO + dI > g->max_deg_both) g->max_deg_both = dO + dI;
        }
    }
    ok = ok && up(&g->off_out, oo.data(), (size_t)n_nodes + 1) == 0 && up(&g->off_in, oi.data(), (size_t)n_nodes + 1) == 0;
    if (!ok) {
        mn_graph_destroy(g);
        return nullptr;
    }
    g->h_off_out.swap(oo);
    g->h_off_in.swap(oi);
    return g;
} MN_GUARD_END(gset_err, MN_NOTHING, nullptr)

extern "C" void mn_graph_retain(mn_graph *g) {
    if (g)
        g->refs.fetch_add(1, std::memory_order_relaxed);
}

extern "C" void mn_graph_destroy(mn_graph *g) {
    if (!g || g->refs.fetch_sub(1, std::memory_order_acq_rel) > 1)
        return;
    (void)hipSetDevice(g->device);
    if (g->stream)
        (void)hipStreamSynchronize(g->stream);
    (void)hipFree(g->off_out); (void)hipFree(g->tgt_out); (void)hipFree(g->off_in); (void)hipFree(g->tgt_in);
    (void)hipFree(g->w_out); (void)hipFree(g->w_in);
    if (g->work)
        lei_work_free(g->work);
    if (g->bfs)
        bfs_work_free(g->bfs);
    if (g->dfs)
        dfs_work_free(g->dfs);
    if (g->sel)
        sel_work_free(g->sel);
    if (g->sp)
        sp_work_free(g->sp);
    if (g->ev0) (void)hipEventDestroy(g->ev0);
    if (g->ev1) (void)hipEventDestroy(g->ev1);
    if (g->stream) (void)hipStreamDestroy(g->stream);
    delete g;
}

extern "C" double mn_graph_last_ms(mn_graph *g) { return g->last_ms; }

// GraphData.out as the host sees it (graph_edge_betweenness emits its rows in this order, src/graph_centrality.c:1172-1182)
extern "C" long long mn_graph_out_edge_count(mn_graph *g) { return g->e_out; }
extern "C" int mn_graph_out_lists(mn_graph *g, int *off, int *tgt) try {
    GCHK(hipSetDevice(g->device));
    memcpy(off, g->h_off_out.data(), ((size_t)g->n + 1) * sizeof(int));
    if (g->e_out)
        GCHK(hipMemcpy(tgt, g->tgt_out, (size_t)g->e_out * sizeof(int), hipMemcpyDeviceToHost));
    return 0;
} MN_GUARD_END(gset_err, MN_NOTHING, -1)
