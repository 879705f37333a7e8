// mn_centrality.hip — the centrality measures over an mn_graph's device-resident CSR, gfx950:
//   mn_graph_betweenness   Brandes, one lane per source
//   mn_graph_closeness     bit-parallel multi-source BFS (unweighted), one lane per source Dijkstra (weighted)
//   mn_graph_degree        one lane per node
#include "mn_graph_int.hpp"
#include "mn_guard.hpp"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>

// ───────────────────────── what the entry points share ─────────────────────────

// One lane per source, and every lane a chain of dependent accesses to its own rows: what hides the latency is the
// number of wavefronts, not their width.  Narrow workgroups (4 to 64 lanes) until the launch has some 4 096 of them —
// 20 000 sources are 5 000 four-lane wavefronts, five per SIMD, instead of 313 full ones on a third of the SIMDs; a
// divergent memory instruction also costs one address cycle per distinct line, so narrow wavefronts lose nothing.
static int lanes_for(int n_src, const char *env) {
    int lanes = 64;
    if (const char *e = getenv(env))
        lanes = std::max(1, std::min(64, atoi(e)));
    else
        while (lanes > 4 && (n_src + lanes - 1) / lanes < 4096)
            lanes >>= 1;
    return lanes;
}

// dpq_pop / dpq_push (:158-212) verbatim — the lazy binary heap of sssp_dijkstra.  `<` going down and `<=` going up decide
// the order in which equal distances leave the heap, which the results depend on.
struct BrDpq {
    int node;
    double dist;
};

DEVI BrDpq dpq_pop(BrDpq *h, int &hs) {
    const BrDpq top = h[0];
    hs--;
    if (hs > 0) {
        h[0] = h[hs];
        int i = 0;
        for (;;) {
            const int left = 2 * i + 1, right = 2 * i + 2;
            int smallest = i;
            if (left < hs && h[left].dist < h[smallest].dist)
                smallest = left;
            if (right < hs && h[right].dist < h[smallest].dist)
                smallest = right;
            if (smallest == i)
                break;
            const BrDpq t = h[i];
            h[i] = h[smallest];
            h[smallest] = t;
            i = smallest;
        }
    }
    return top;
}

// false: the heap is full (cap entries) and nothing was written
DEVI bool dpq_push(BrDpq *h, int &hs, long long cap, int node, double dist) {
    if (hs >= cap)
        return false;
    int i = hs++;
    h[i].node = node;
    h[i].dist = dist;
    while (i > 0) {
        const int parent = (i - 1) / 2;
        if (h[parent].dist <= h[i].dist)
            break;
        const BrDpq t = h[parent];
        h[parent] = h[i];
        h[i] = t;
        i = parent;
    }
    return true;
}

// ───────────────────────── Brandes betweenness (src/graph_centrality.c:260-505) ─────────────────────────
// The reference runs one single-source shortest-path pass per source — BFS for unweighted graphs, Dijkstra with a lazy binary
// heap for weighted ones, predecessor lists in discovery order — then the dependency accumulation in reverse stack order,
// and adds every source's result to CB / EB in source order (f64: the order of those additions is part of the result).
// Sources are independent, so the device runs them side by side: ONE LANE PER SOURCE replays the reference's pass verbatim
// on that source's own scratch rows (queue, stack, predecessor lists, heap — the same control flow, hence the same
// stack order, predecessor order and f64 operations), and k_brandes_accumulate then folds the sources of the chunk into
// CB[w] / EB[v][w] in source order, one lane per target w (a cell is only ever written by w's lane).  The dependency of w
// at the moment the reference pops it is its final value, so the flow (sigma[v] / sigma[w]) * (1 + delta[w]) is recomputed
// there from the stored sigma / delta with the same operands.  Divergent by construction (64 different traversals per
// wavefront): this trades SIMD efficiency for bit-exact reference semantics; throughput comes from thousands of sources
// in flight.
struct BrCell {
    double dist, sigma, delta;
    int pcnt, pad;
};
struct BrArgs {
    DevGraph g;
    int use_out, use_in, weighted;
    int n_src;           // sources in this chunk
    const int *sources;  // [n_src]
    const int *poff;     // [N+1] predecessor-list slots per node (static: one per incident traversed edge)
    long long P;         // poff[N]
    long long heap_cap;  // Dijkstra: entries per source
    BrCell *cell;        // [n_src][N]   what a pass keeps per node, side by side (one line per touch of a node instead of three)
    int *stack, *queue;  // [n_src][N]   (queue doubles as Dijkstra's settled flags)
    int *pitems;                  // [n_src][P]
    BrDpq *heap;                  // [n_src][heap_cap]
    int *overflow;
};

DEVI bool br_double_eq(double a, double b) { return fabs(a - b) < 1e-10 * fmax(1.0, fabs(b)); } // :215-217

__global__ void __launch_bounds__(64) k_brandes_sources(BrArgs a) {
    const int si = blockIdx.x * blockDim.x + threadIdx.x;
    if (si >= a.n_src)
        return;
    const int N = a.g.n, src = a.sources[si];
    BrCell *c = a.cell + (size_t)si * N;
    int *stack = a.stack + (size_t)si * N, *queue = a.queue + (size_t)si * N;
    int *pitems = a.pitems + (size_t)si * a.P;
    for (int i = 0; i < N; i++) {
        c[i] = BrCell{-1.0, 0.0, 0.0, 0, 0};
        if (a.weighted)
            queue[i] = 0; // (Dijkstra's settled flags; the BFS writes a queue position before it reads it)
    }
    c[src].dist = 0.0;
    c[src].sigma = 1.0;
    int ss = 0;
    if (!a.weighted) { // sssp_bfs, :263-315
        int qh = 0, qt = 0;
        queue[qt++] = src;
        while (qh < qt) {
            const int v = queue[qh++];
            stack[ss++] = v;
            for (int pass = 0; pass < 2; pass++) {
                if (pass == 0 ? !a.use_out : !a.use_in)
                    continue;
                const int *off = pass ? a.g.off_in : a.g.off_out, *tgt = pass ? a.g.tgt_in : a.g.tgt_out;
                for (int e = off[v]; e < off[v + 1]; e++) {
                    const int w = tgt[e];
                    if (c[w].dist < 0) {
                        c[w].dist = c[v].dist + 1.0;
                        queue[qt++] = w;
                    }
                    if (br_double_eq(c[w].dist, c[v].dist + 1.0)) {
                        const int pc = c[w].pcnt;
                        if (pc == 0 || pitems[a.poff[w] + pc - 1] != v) {
                            c[w].sigma += c[v].sigma;
                            pitems[a.poff[w] + pc] = v;
                            c[w].pcnt = pc + 1;
                        }
                    }
                }
            }
        }
    } else { // sssp_dijkstra, :321-378
        BrDpq *h = a.heap + (size_t)si * a.heap_cap;
        int hs = 0;
        int *settled = queue;
        h[hs].node = src;
        h[hs].dist = 0.0;
        hs++;
        while (hs > 0) {
            const int v = dpq_pop(h, hs).node;
            if (settled[v])
                continue;
            settled[v] = 1;
            stack[ss++] = v;
            for (int pass = 0; pass < 2; pass++) {
                if (pass == 0 ? !a.use_out : !a.use_in)
                    continue;
                const int *off = pass ? a.g.off_in : a.g.off_out, *tgt = pass ? a.g.tgt_in : a.g.tgt_out;
                const double *wt = pass ? a.g.w_in : a.g.w_out;
                for (int e = off[v]; e < off[v + 1]; e++) {
                    const int w = tgt[e];
                    const double nd = c[v].dist + (wt ? wt[e] : 1.0);
                    if (c[w].dist < 0 || nd < c[w].dist - 1e-10) {
                        c[w].dist = nd;
                        c[w].sigma = c[v].sigma;
                        pitems[a.poff[w]] = v;
                        c[w].pcnt = 1;
                        if (!dpq_push(h, hs, a.heap_cap, w, nd)) {
                            *a.overflow = 1;
                            return;
                        }
                    } else if (br_double_eq(nd, c[w].dist)) {
                        const int pc = c[w].pcnt;
                        if (pc == 0 || pitems[a.poff[w] + pc - 1] != v) {
                            if (pc >= a.poff[w + 1] - a.poff[w]) { // (cannot happen: one slot per incident edge)
                                *a.overflow = 1;
                                return;
                            }
                            c[w].sigma += c[v].sigma;
                            pitems[a.poff[w] + pc] = v;
                            c[w].pcnt = pc + 1;
                        }
                    }
                }
            }
        }
    }
    // dependency accumulation in reverse stack order (:448-462)
    while (ss > 0) { // (delta is zero from the start: the passes above never touch it)
        const int w = stack[--ss];
        const int pc = c[w].pcnt;
        for (int pi = 0; pi < pc; pi++) {
            const int v = pitems[a.poff[w] + pi];
            if (c[w].sigma > 0) {
                const double flow = (c[v].sigma / c[w].sigma) * (1.0 + c[w].delta);
                c[v].delta += flow;
            }
        }
    }
}

// CB[w] += delta_s[w] (w != s) and EB[v*N + w] += flow, sources of the chunk in order; one lane per target w
__global__ void k_brandes_accumulate(BrArgs a, double *CB, double *EB) {
    const int w = blockIdx.x * blockDim.x + threadIdx.x;
    const int N = a.g.n;
    if (w >= N)
        return;
    double cb = CB[w];
    for (int si = 0; si < a.n_src; si++) {
        const BrCell *c = a.cell + (size_t)si * N;
        const double dw = c[w].delta;
        if (EB) {
            const int pc = c[w].pcnt;
            const int *items = a.pitems + (size_t)si * a.P + a.poff[w];
            const double sw = c[w].sigma;
            for (int pi = 0; pi < pc; pi++) {
                const int v = items[pi];
                if (sw > 0)
                    EB[(size_t)v * N + w] += (c[v].sigma / sw) * (1.0 + dw);
            }
        }
        if (w != a.sources[si])
            cb += dw;
    }
    CB[w] = cb;
}

__global__ void k_scale_d(double *x, long long n, double mul, double div1, double div2) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n)
        return;
    double v = x[i];
    if (mul != 1.0)
        v *= mul;
    if (div1 != 1.0)
        v /= div1;
    if (div2 != 1.0)
        v /= div2;
    x[i] = v;
}

extern "C" int mn_graph_betweenness(mn_graph *g, int direction, int auto_approx, int normalized, double *cb_out, double *eb_out) try {
    GCHK(hipSetDevice(g->device));
    const int N = g->n;
    if (N == 0)
        return 0;
    int use_out, use_in; // :281-282
    if (graph_direction("mn_graph_betweenness", direction, &use_out, &use_in))
        return -1;
    hipStream_t st = g->stream;
    // source set (:417-433)
    std::vector<int> sources;
    double scale = 1.0;
    if (auto_approx > 0 && N > auto_approx) {
        const int want = (int)ceil(sqrt((double)N));
        int n_sources = want < 1 ? 1 : want;
        int step = N / n_sources;
        if (step < 1)
            step = 1;
        for (int i = 0; i < N && (int)sources.size() < want; i += step)
            sources.push_back(i);
        scale = (double)N / (double)sources.size();
    } else {
        for (int i = 0; i < N; i++)
            sources.push_back(i);
    }
    // predecessor slots: one per traversed edge arriving at the node
    std::vector<int> tgt_o((size_t)g->e_out), tgt_i((size_t)g->e_in), poff((size_t)N + 1, 0);
    if (g->e_out)
        GCHK(hipMemcpy(tgt_o.data(), g->tgt_out, (size_t)g->e_out * sizeof(int), hipMemcpyDeviceToHost));
    if (g->e_in)
        GCHK(hipMemcpy(tgt_i.data(), g->tgt_in, (size_t)g->e_in * sizeof(int), hipMemcpyDeviceToHost));
    long long e_trav = 0;
    if (use_out)
        for (int x : tgt_o) {
            poff[(size_t)x + 1]++;
            e_trav++;
        }
    if (use_in)
        for (int x : tgt_i) {
            poff[(size_t)x + 1]++;
            e_trav++;
        }
    for (int i = 0; i < N; i++)
        poff[(size_t)i + 1] += poff[(size_t)i];
    const long long P = poff[(size_t)N] > 0 ? poff[(size_t)N] : 1;
    const long long heap_cap = g->weighted ? e_trav + 2 : 1;
    // chunk of sources that fits the scratch budget
    const size_t per_src = (size_t)N * (sizeof(BrCell) + 2 * sizeof(int)) + (size_t)P * sizeof(int) + (size_t)heap_cap * sizeof(BrDpq);
    // Half of what the device has free (round 4): the lanes of a launch are the only parallelism there is, and at the 8 GB of
    // rounds 2-3 a 20 000-node graph went through in six launches of 58 wavefronts each on a chip of 1 024 SIMDs.
    const size_t eb_bytes = eb_out ? (size_t)N * N * sizeof(double) : 0; // (allocated after the scratch: leave it its room)
    const size_t budget = scratch_budget("MN_BRANDES_SCRATCH_MB", eb_bytes);
    int chunk = (int)std::max<size_t>(1, std::min<size_t>(sources.size(), budget / per_src));
    DevArena scr;
    BrArgs a;
    memset(&a, 0, sizeof(a));
    a.g = dev_graph_of(g);
    a.use_out = use_out;
    a.use_in = use_in;
    a.weighted = g->weighted ? 1 : 0;
    a.P = P;
    a.heap_cap = heap_cap;
    int *d_sources = scr.alloc<int>((size_t)chunk), *d_poff = scr.alloc<int>((size_t)N + 1);
    a.cell = scr.alloc<BrCell>((size_t)chunk * N);
    a.stack = scr.alloc<int>((size_t)chunk * N);
    a.queue = scr.alloc<int>((size_t)chunk * N);
    a.pitems = scr.alloc<int>((size_t)chunk * P);
    a.heap = scr.alloc<BrDpq>((size_t)chunk * heap_cap);
    a.overflow = scr.alloc<int>(1);
    double *d_cb = scr.alloc<double>((size_t)N);
    double *d_eb = eb_out ? scr.alloc<double>((size_t)N * N) : nullptr;
    if (!d_sources || !d_poff || !a.cell || !a.stack || !a.queue || !a.pitems || !a.heap ||
        !a.overflow || !d_cb || (eb_out && !d_eb)) {
        gset_err("mn_graph_betweenness: out of device memory (N = %d%s)", N, eb_out ? ", dense N x N edge matrix as in the reference" : "");
        return -1;
    }
    a.sources = d_sources;
    a.poff = d_poff;
    GCHK(hipMemcpyAsync(d_poff, poff.data(), ((size_t)N + 1) * sizeof(int), hipMemcpyHostToDevice, st));
    GCHK(hipMemsetAsync(d_cb, 0, (size_t)N * sizeof(double), st));
    GCHK(hipMemsetAsync(a.overflow, 0, sizeof(int), st));
    if (d_eb)
        GCHK(hipMemsetAsync(d_eb, 0, (size_t)N * N * sizeof(double), st));
    GCHK(hipEventRecord(g->ev0, st));
    for (size_t s0 = 0; s0 < sources.size(); s0 += (size_t)chunk) {
        a.n_src = (int)std::min<size_t>((size_t)chunk, sources.size() - s0);
        GCHK(hipMemcpyAsync(d_sources, sources.data() + s0, (size_t)a.n_src * sizeof(int), hipMemcpyHostToDevice, st));
        const int lanes = lanes_for(a.n_src, "MN_BRANDES_LANES");
        hipLaunchKernelGGL(k_brandes_sources, dim3((a.n_src + lanes - 1) / lanes), dim3(lanes), 0, st, a);
        hipLaunchKernelGGL(k_brandes_accumulate, dim3((N + 255) / 256), dim3(256), 0, st, a, d_cb, d_eb);
        GCHK(hipStreamSynchronize(st)); // (the host vector `sources` chunk must outlive the copy; also bounds the queue)
    }
    // approximation scale, undirected halving, normalisation — in the reference's order (:466-498)
    const int undirected = direction == 0;
    const double half = undirected ? 2.0 : 1.0;
    double norm = 1.0;
    if (normalized && N > 2)
        norm = undirected ? (double)(N - 1) * (double)(N - 2) / 2.0 : (double)(N - 1) * (double)(N - 2);
    hipLaunchKernelGGL(k_scale_d, dim3((N + 255) / 256), dim3(256), 0, st, d_cb, (long long)N, scale, half, norm);
    if (d_eb)
        hipLaunchKernelGGL(k_scale_d, dim3((unsigned)(((long long)N * N + 255) / 256)), dim3(256), 0, st, d_eb, (long long)N * N, scale,
                           half, norm);
    if (graph_mark(g))
        return -1;
    int ovf = 0;
    GCHK(hipMemcpyAsync(&ovf, a.overflow, sizeof(int), hipMemcpyDeviceToHost, st));
    GCHK(hipMemcpyAsync(cb_out, d_cb, (size_t)N * sizeof(double), hipMemcpyDeviceToHost, st));
    if (d_eb)
        GCHK(hipMemcpyAsync(eb_out, d_eb, (size_t)N * N * sizeof(double), hipMemcpyDeviceToHost, st));
    GCHK(hipStreamSynchronize(st));
    if (ovf) {
        gset_err("mn_graph_betweenness: scratch overflow");
        return -1;
    }
    graph_note_ms(g);
    return 0;
} MN_GUARD_END(gset_err, MN_NOTHING, -1)

// ───────────────────────── closeness and degree (src/graph_centrality.c:1316-1455 and :591-686) ─────────────────────────
// clo_filter runs one shortest-path pass per node and keeps of it only the distances: closeness[s] = reachable / sum_dist,
// times reachable / (N - 1) when normalized (Wasserman-Faust).
//
// Unweighted graphs: every distance of sssp_bfs is an integer-valued double, so sum_dist is a sum of integers below 2^53 —
// exact in ANY order, and equal to  sum over levels of  level x (nodes first reached at that level).  The traversal order
// therefore does not enter the result and the passes need not be replayed one lane per source: the device runs a
// level-synchronous BIT-PARALLEL multi-source BFS.  A 64-bit word holds one bit per source of a batch of 64 sources; per node
// and batch there are the words seen / frontier / next, laid out [node][batch] so that the 64 lanes of a wavefront working
// on one node touch 64 adjacent words.
//   k_clo_expand   one wavefront per (node v, 64 batches): the neighbour list of v is read once, wave-uniformly, and
//                  frontier[v] & ~seen[w] is OR-ed into next[w] — the atomics of one neighbour land in one 512-byte run
//   k_clo_update   one workgroup per 64 nodes x 64 batches: new = next & ~seen, seen |= new, frontier = new, next = 0 with
//                  lanes over batches; the new words go through LDS and are read back with lanes over NODES, so that 64
//                  ballots + popcounts give, per source of the batch, how many of the 64 nodes it just reached: lane `bit`
//                  adds that count to reachable[source] and count x level to sum_dist[source] (two 64-bit atomics per
//                  (64 nodes, source) that gained anything, none per (node, bit))
// Sources are processed in chunks of batches under a scratch budget (24 bytes per node per batch); a level ends when the
// update kernel saw no new bit in any batch.
//
// Weighted graphs have no such freedom (the 1e-10 slack of sssp_dijkstra and f64 sums of non-integers): ONE LANE PER SOURCE
// replays sssp_dijkstra with dpq_push / dpq_pop verbatim, as k_brandes_sources does, but without sigma, predecessor lists
// and stack — the distances depend on none of them — then sums dist[] in index order and applies the same two f64 operations.
typedef unsigned long long clo_word;

DEVI double clo_value(long long reachable, double sum_dist, int normalized, int N) { // :1426-1433
    if (!(reachable > 0 && sum_dist > 0))
        return 0.0;
    double cc = (double)reachable / sum_dist;
    if (normalized && N > 1)
        cc *= (double)reachable / (double)(N - 1);
    return cc;
}

// the chunk holds the batches b0 .. b0 + B - 1; source s = 64 * batch + bit starts at node s
__global__ void __launch_bounds__(256) k_clo_init(int N, int B, long long b0, clo_word *seen, clo_word *frontier, clo_word *next) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)N * B)
        return;
    const int v = (int)(i / B), b = (int)(i % B);
    const clo_word w = (long long)(v >> 6) == b0 + b ? (clo_word)1 << (v & 63) : 0;
    seen[i] = w;
    frontier[i] = w;
    next[i] = 0;
}

__global__ void __launch_bounds__(256) k_clo_expand(DevGraph g, int use_out, int use_in, int B, const clo_word *seen,
                                                    const clo_word *frontier, clo_word *next) {
    const int b = blockIdx.y * 64 + (threadIdx.x & 63);
    for (int vv = blockIdx.x * 4 + (threadIdx.x >> 6); vv < g.n; vv += gridDim.x * 4) { // (vv is the same in all 64 lanes)
        const int v = __builtin_amdgcn_readfirstlane(vv);
        const clo_word f = b < B ? frontier[(size_t)v * B + b] : 0;
        if (__ballot(f != 0) == 0)
            continue;
        for (int pass = 0; pass < 2; pass++) { // out[v], then in[v], as sssp_bfs (:286-289); the order does not matter here
            if (pass == 0 ? !use_out : !use_in)
                continue;
            const int *off = pass ? g.off_in : g.off_out, *tgt = pass ? g.tgt_in : g.tgt_out;
            const int e1 = off[v + 1];
            for (int e = off[v]; e < e1; e++) {
                const int w = tgt[e];
                if (f != 0) {
                    const size_t i = (size_t)w * B + b;
                    const clo_word m = f & ~seen[i];
                    if (m != 0)
                        atomicOr(&next[i], m);
                }
            }
        }
    }
}

#define CLO_TILE_PAD 65 // words per LDS row: the column reads of the counting pass then spread over the banks
__global__ void __launch_bounds__(256) k_clo_update(int N, int B, long long b0, long long level, clo_word *seen, clo_word *frontier,
                                                    clo_word *next, unsigned long long *reachable, unsigned long long *sum_dist,
                                                    int *any_new) {
    __shared__ clo_word tile[64 * CLO_TILE_PAD];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int v0 = blockIdx.x * 64, bb = blockIdx.y * 64;
    const int b = bb + lane;
    int any = 0;
    for (int r = wv; r < 64; r += 4) { // lanes over batches
        const int v = v0 + r;
        clo_word nw = 0;
        if (v < N && b < B) {
            const size_t i = (size_t)v * B + b;
            const clo_word nx = next[i], sn = seen[i];
            nw = nx & ~sn;
            if (nw != 0)
                seen[i] = sn | nw;
            frontier[i] = nw;
            if (nx != 0)
                next[i] = 0;
        }
        tile[r * CLO_TILE_PAD + lane] = nw;
        any |= nw != 0;
    }
    if (!__syncthreads_or(any))
        return;
    if (threadIdx.x == 0)
        *any_new = 1;
    for (int c = wv * 16; c < wv * 16 + 16; c++) { // lanes over nodes: one batch per step
        if (bb + c >= B)
            break;
        const clo_word x = tile[lane * CLO_TILE_PAD + c];
        if (__ballot(x != 0) == 0)
            continue;
        unsigned long long cnt = 0;
#pragma unroll
        for (int bit = 0; bit < 64; bit++) {
            const unsigned long long m = __ballot((x >> bit) & 1);
            if (lane == bit)
                cnt = (unsigned long long)__popcll(m);
        }
        if (cnt != 0) {
            const size_t s = (size_t)(b0 + bb + c) * 64 + lane;
            atomicAdd(&reachable[s], cnt);
            atomicAdd(&sum_dist[s], cnt * (unsigned long long)level);
        }
    }
}

__global__ void __launch_bounds__(256) k_clo_finish(int N, int normalized, const unsigned long long *reachable,
                                                    const unsigned long long *sum_dist, double *cc) {
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s < N)
        cc[s] = clo_value((long long)reachable[s], (double)sum_dist[s], normalized, N);
}

struct CloArgs {
    DevGraph g;
    int use_out, use_in, normalized;
    int s0, n_src;       // this chunk's sources are s0 .. s0 + n_src - 1
    long long heap_cap;  // entries per source
    double *dist;        // [n_src][N]
    int *settled;        // [n_src][N]
    BrDpq *heap;         // [n_src][heap_cap]
    double *cc;          // [N]
    int *overflow;
};

__global__ void __launch_bounds__(64) k_clo_dijkstra(CloArgs a) {
    const int si = blockIdx.x * blockDim.x + threadIdx.x;
    if (si >= a.n_src)
        return;
    const int N = a.g.n, src = a.s0 + si;
    double *dist = a.dist + (size_t)si * N;
    int *settled = a.settled + (size_t)si * N;
    for (int i = 0; i < N; i++) {
        dist[i] = -1.0;
        settled[i] = 0;
    }
    dist[src] = 0.0;
    // sssp_dijkstra, :321-378
    BrDpq *h = a.heap + (size_t)si * a.heap_cap;
    int hs = 0;
    h[hs].node = src;
    h[hs].dist = 0.0;
    hs++;
    while (hs > 0) {
        const int v = dpq_pop(h, hs).node;
        if (settled[v])
            continue;
        settled[v] = 1;
        for (int pass = 0; pass < 2; pass++) {
            if (pass == 0 ? !a.use_out : !a.use_in)
                continue;
            const int *off = pass ? a.g.off_in : a.g.off_out, *tgt = pass ? a.g.tgt_in : a.g.tgt_out;
            const double *wt = pass ? a.g.w_in : a.g.w_out;
            for (int e = off[v]; e < off[v + 1]; e++) {
                const int w = tgt[e];
                const double nd = dist[v] + (wt ? wt[e] : 1.0);
                if (dist[w] < 0 || nd < dist[w] - 1e-10) {
                    dist[w] = nd;
                    if (!dpq_push(h, hs, a.heap_cap, w, nd)) {
                        *a.overflow = 1;
                        return;
                    }
                }
            }
        }
    }
    double sum_dist = 0.0; // :1417-1424
    int reachable = 0;
    for (int i = 0; i < N; i++)
        if (i != src && dist[i] >= 0) {
            sum_dist += dist[i];
            reachable++;
        }
    a.cc[src] = clo_value(reachable, sum_dist, a.normalized, N);
}

extern "C" int mn_graph_closeness(mn_graph *g, int direction, int normalized, double *out) try {
    GCHK(hipSetDevice(g->device));
    const int N = g->n;
    if (N == 0)
        return 0;
    int use_out, use_in; // :278-279
    if (graph_direction("mn_graph_closeness", direction, &use_out, &use_in))
        return -1;
    if (N > (1 << 26)) { // (N - 1)^2 bounds sum_dist: past this it leaves the range in which every integer is a double
        gset_err("mn_graph_closeness: more than 2^26 nodes (N = %d)", N);
        return -1;
    }
    hipStream_t st = g->stream;
    DevArena scr;
    const DevGraph dg = dev_graph_of(g);
    const size_t budget = scratch_budget("MN_CLOSENESS_SCRATCH_MB", 0);
    double *d_cc = scr.alloc<double>((size_t)N);
    int *d_flag = scr.alloc<int>(1);
    int ovf = 0;
    if (!g->weighted) {
        const long long nb_total = ((long long)N + 63) / 64;
        const size_t per_batch = (size_t)N * 3 * sizeof(clo_word);
        // (at most 2^30 words per array: every launch below then stays inside the 2^32 threads a grid may have)
        const int B = (int)scratch_chunk((size_t)nb_total, budget, per_batch, ((size_t)1 << 30) / (size_t)N);
        clo_word *seen = scr.alloc<clo_word>((size_t)N * B);
        clo_word *frontier = scr.alloc<clo_word>((size_t)N * B);
        clo_word *next = scr.alloc<clo_word>((size_t)N * B);
        unsigned long long *reach = scr.alloc<unsigned long long>((size_t)nb_total * 64);
        unsigned long long *sum = scr.alloc<unsigned long long>((size_t)nb_total * 64);
        if (!d_cc || !d_flag || !seen || !frontier || !next || !reach || !sum) {
            gset_err("mn_graph_closeness: out of device memory (N = %d, %d batches of 64 sources at once)", N, B);
            return -1;
        }
        GCHK(hipMemsetAsync(reach, 0, (size_t)nb_total * 64 * sizeof(unsigned long long), st));
        GCHK(hipMemsetAsync(sum, 0, (size_t)nb_total * 64 * sizeof(unsigned long long), st));
        GCHK(hipEventRecord(g->ev0, st));
        for (long long b0 = 0; b0 < nb_total; b0 += B) {
            const int Bc = (int)std::min<long long>(B, nb_total - b0);
            const size_t words = (size_t)N * Bc;
            hipLaunchKernelGGL(k_clo_init, dim3((unsigned)((words + 255) / 256)), dim3(256), 0, st, N, Bc, b0, seen, frontier, next);
            const dim3 grid_e(std::min((N + 3) / 4, 1 << 16), (Bc + 63) / 64), grid_u((N + 63) / 64, (Bc + 63) / 64);
            for (long long level = 1; level <= N; level++) { // (a level past N - 1 cannot add a bit)
                GCHK(hipMemsetAsync(d_flag, 0, sizeof(int), st));
                hipLaunchKernelGGL(k_clo_expand, grid_e, dim3(256), 0, st, dg, use_out, use_in, Bc, seen, frontier, next);
                hipLaunchKernelGGL(k_clo_update, grid_u, dim3(256), 0, st, N, Bc, b0, level, seen, frontier, next, reach, sum, d_flag);
                int any_new = 0;
                GCHK(hipMemcpyAsync(&any_new, d_flag, sizeof(int), hipMemcpyDeviceToHost, st));
                GCHK(hipStreamSynchronize(st));
                if (!any_new)
                    break;
            }
        }
        hipLaunchKernelGGL(k_clo_finish, dim3((N + 255) / 256), dim3(256), 0, st, N, normalized ? 1 : 0, reach, sum, d_cc);
    } else {
        const long long e_trav = (use_out ? g->e_out : 0) + (use_in ? g->e_in : 0);
        CloArgs a;
        memset(&a, 0, sizeof(a));
        a.g = dg;
        a.use_out = use_out;
        a.use_in = use_in;
        a.normalized = normalized ? 1 : 0;
        a.heap_cap = e_trav + 2;
        const size_t per_src = (size_t)N * (sizeof(double) + sizeof(int)) + (size_t)a.heap_cap * sizeof(BrDpq);
        const int chunk = (int)std::max<size_t>(1, std::min<size_t>((size_t)N, budget / per_src));
        a.dist = scr.alloc<double>((size_t)chunk * N);
        a.settled = scr.alloc<int>((size_t)chunk * N);
        a.heap = scr.alloc<BrDpq>((size_t)chunk * a.heap_cap);
        a.cc = d_cc;
        a.overflow = d_flag;
        if (!d_cc || !d_flag || !a.dist || !a.settled || !a.heap) {
            gset_err("mn_graph_closeness: out of device memory (N = %d, %d sources at once)", N, chunk);
            return -1;
        }
        GCHK(hipMemsetAsync(d_flag, 0, sizeof(int), st));
        GCHK(hipEventRecord(g->ev0, st));
        for (int s0 = 0; s0 < N; s0 += chunk) {
            a.s0 = s0;
            a.n_src = std::min(chunk, N - s0);
            const int lanes = lanes_for(a.n_src, "MN_CLOSENESS_LANES");
            hipLaunchKernelGGL(k_clo_dijkstra, dim3((a.n_src + lanes - 1) / lanes), dim3(lanes), 0, st, a);
        }
        GCHK(hipMemcpyAsync(&ovf, d_flag, sizeof(int), hipMemcpyDeviceToHost, st));
    }
    if (graph_mark(g))
        return -1;
    GCHK(hipMemcpyAsync(out, d_cc, (size_t)N * sizeof(double), hipMemcpyDeviceToHost, st));
    GCHK(hipStreamSynchronize(st));
    if (ovf) {
        gset_err("mn_graph_closeness: scratch overflow");
        return -1;
    }
    graph_note_ms(g);
    return 0;
} MN_GUARD_END(gset_err, MN_NOTHING, -1)

// deg_filter's loop (:667-680): one lane per node, the two lists summed in list order
__global__ void __launch_bounds__(256) k_degree(DevGraph g, int normalized, double *in_deg, double *out_deg, double *degree,
                                                double *centrality) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= g.n)
        return;
    double in = 0, out = 0;
    for (int e = g.off_out[i]; e < g.off_out[i + 1]; e++)
        out += g.w_out ? g.w_out[e] : 1.0;
    for (int e = g.off_in[i]; e < g.off_in[i + 1]; e++)
        in += g.w_in ? g.w_in[e] : 1.0;
    const double total = in + out;
    double cent = total;
    if (normalized && g.n > 1)
        cent = total / (double)(g.n - 1);
    in_deg[i] = in;
    out_deg[i] = out;
    degree[i] = total;
    centrality[i] = cent;
}

extern "C" int mn_graph_degree(mn_graph *g, int normalized, double *in_deg, double *out_deg, double *degree, double *centrality) try {
    GCHK(hipSetDevice(g->device));
    const int N = g->n;
    if (N == 0)
        return 0;
    hipStream_t st = g->stream;
    DevArena scr;
    double *d = scr.alloc<double>((size_t)4 * N);
    if (!d) {
        gset_err("mn_graph_degree: out of device memory (N = %d)", N);
        return -1;
    }
    hipLaunchKernelGGL(k_degree, dim3((N + 255) / 256), dim3(256), 0, st, dev_graph_of(g), normalized ? 1 : 0, d, d + N,
                       d + 2 * (size_t)N, d + 3 * (size_t)N);
    GCHK(hipGetLastError());
    double *dst[4] = {in_deg, out_deg, degree, centrality};
    for (int k = 0; k < 4; k++)
        if (dst[k])
            GCHK(hipMemcpyAsync(dst[k], d + (size_t)k * N, (size_t)N * sizeof(double), hipMemcpyDeviceToHost, st));
    GCHK(hipStreamSynchronize(st));
    return 0;
} MN_GUARD_END(gset_err, MN_NOTHING, -1)
