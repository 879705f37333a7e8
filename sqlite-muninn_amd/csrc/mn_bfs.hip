// mn_bfs.hip — breadth-first traversal over an mn_graph's device-resident CSR, gfx950:
//   mn_graph_bfs        run_bfs (src/graph_tvf.c:230-309) for many start nodes at once, rows in the reference's queue order
//   mn_graph_bfs_rows   the (node, depth, parent) rows of the last call
//
// The reference pops a queue: a node's neighbours (its out-list, then its in-list, each in table-row order) are pushed when
// first seen, with the popped node as parent.  The queue order is therefore level by level, and inside a level a node stands
// at the rank of the FIRST edge that reaches it when the edges of the previous level are enumerated in (parent's position
// in its level, index in the parent's list) order.  That enumeration index is a number, so "first" is a minimum and no
// arrival order enters the answer:
//
//   per level, for the frontier entries of every seed of the chunk (the pool's last slice, in (seed, position) order):
//     scan       inclusive scan of the entries' degrees: edge e of the level belongs to the entry i with
//                iscan[i-1] <= e < iscan[i]; e_local = e - (first edge of the entry's seed) numbers a seed's own edges
//     k_claim    one lane per EDGE (a hub's list is spread over lanes and workgroups; a binary search in iscan finds the
//                entry): plain load of key[slot][v]; 0 = visited, nothing to do; else atomicMin(key, e_local + 1)
//     k_count    the same enumeration in fixed contiguous ranges, one per workgroup: an edge has won iff
//                key[slot][v] == e_local + 1; per-range win counts and the level's total
//     (host)     reads the total: stops at 0, grows the pool if it has to
//     k_emit     the same ranges again: range base + the running in-range prefix of the win flags is the node's position in the
//                next level; (v, u, slot, depth) is written there and the winner sets key = 0 — no other edge compares
//                equal to a winner's claim, and claims are >= 1, so no second pass is needed and none is left behind
//
//   key[slot][node] is 32 bits: 0 visited, 0xFFFFFFFF untouched, anything else this level's claim.  It is filled once per
//   allocation; after a chunk only the entries the chunk's output names are reset.  A stable sort of the pool by seed slot
//   (level slices keep their order) gives the seed-major rows.
#include "mn_guard.hpp"
#include "mn_prim.hpp"
#include "mn_traverse.hpp"

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>
#include <rocprim/iterator/transform_iterator.hpp>

#include <algorithm>
#include <cstring>

typedef unsigned long long bfs_u64;

#define BFS_UNTOUCHED 0xFFFFFFFFu
#define BFS_BLOCK 256
#define BFS_MAX_RANGES 2048                      // workgroups of k_count / k_emit: one contiguous edge range each
#define BFS_BYTES_PER_NODE_SLOT ((size_t)64)     // scratch a seed slot may come to need, per node (include/muninn_hip.h)

struct BfsWork {
    DevBuf<unsigned> key;   // [slots][n], slots = key.cap / n
    bool key_clean = false; // every entry is BFS_UNTOUCHED
    DevBuf<int> p_node, p_parent, p_slot, p_depth; // the pool: four columns of pool_cap() entries
    DevBuf<bfs_u64> iscan;       // inclusive degree sums of the frontier
    DevBuf<bfs_u64> seg_e;       // [slots] first edge of a seed's part of the level's enumeration
    DevBuf<int> d_seeds;         // [slots]
    DevBuf<long long> d_rowoff;  // [slots]
    DevBuf<unsigned> range_cnt;  // [BFS_MAX_RANGES]
    DevBuf<bfs_u64> tot;         // [0] edges of the level, [1] wins of the level, [2] edges scanned so far
    DevBuf<char> tmp;            // rocPRIM's
    TravRows rows;               // of the last call
    size_t pool_cap() const { return std::min(std::min(p_node.cap, p_parent.cap), std::min(p_slot.cap, p_depth.cap)); }
};

void bfs_work_free(BfsWork *w) { delete w; }

// ───────────────────────── kernels ─────────────────────────

struct BfsArgs {
    DevGraph g;
    int use_out, use_in;
    unsigned *key;
    int *p_node, *p_parent, *p_slot, *p_depth;
    long long f0, F;      // the frontier is pool[f0 .. f0 + F)
    const bfs_u64 *iscan; // [F]
    const bfs_u64 *seg_e;
    unsigned *range_cnt;
    bfs_u64 *tot;
    int depth;            // of the nodes this level discovers
};

struct BfsDegOf { // degree of a frontier node in the traversal's direction
    const int *off_out, *off_in;
    int use_out, use_in;
    __host__ __device__ bfs_u64 operator()(int u) const {
        bfs_u64 d = 0;
        if (use_out)
            d += (bfs_u64)(off_out[u + 1] - off_out[u]);
        if (use_in)
            d += (bfs_u64)(off_in[u + 1] - off_in[u]);
        return d;
    }
};

__global__ void __launch_bounds__(BFS_BLOCK) k_bfs_seed(int S, int n, const int *seeds, unsigned *key, int *p_node, int *p_parent,
                                                        int *p_slot, int *p_depth, bfs_u64 *tot) {
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s == 0)
        tot[2] = 0;
    if (s >= S)
        return;
    const int u = seeds[s];
    p_node[s] = u;
    p_parent[s] = -1;
    p_slot[s] = s;
    p_depth[s] = 0;
    key[(size_t)s * n + u] = 0;
}

// where each seed's edges start in the level's enumeration; the level's edge total
__global__ void __launch_bounds__(BFS_BLOCK) k_bfs_segments(BfsArgs a, bfs_u64 *seg_e) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.F)
        return;
    const int slot = a.p_slot[a.f0 + i];
    if (i == 0 || a.p_slot[a.f0 + i - 1] != slot)
        seg_e[slot] = i ? a.iscan[i - 1] : 0;
    if (i == a.F - 1) {
        const bfs_u64 E = a.iscan[i];
        a.tot[0] = E;
        a.tot[1] = 0;
        a.tot[2] += E;
    }
}

struct BfsEdge {
    int u, v;
    unsigned claim; // e_local + 1
    size_t k;       // index into key
};

// edge e of the level's enumeration: the frontier entry it belongs to, its target, its seed's key word and its claim value
DEVI BfsEdge bfs_edge(const BfsArgs &a, bfs_u64 e) {
    long long lo = 0, hi = a.F; // first entry whose inclusive sum exceeds e (entries without edges are stepped over)
    while (lo < hi) {
        const long long mid = (lo + hi) >> 1;
        if (a.iscan[mid] > e)
            hi = mid;
        else
            lo = mid + 1;
    }
    const bfs_u64 first = lo ? a.iscan[lo - 1] : 0;
    int j = (int)(e - first);
    BfsEdge x;
    x.u = a.p_node[a.f0 + lo];
    const int slot = a.p_slot[a.f0 + lo];
    const int d_out = a.use_out ? a.g.off_out[x.u + 1] - a.g.off_out[x.u] : 0;
    if (j < d_out) // the out-list first, then the in-list (:284-297)
        x.v = a.g.tgt_out[a.g.off_out[x.u] + j];
    else
        x.v = a.g.tgt_in[a.g.off_in[x.u] + (j - d_out)];
    x.claim = (unsigned)(e - a.seg_e[slot]) + 1u;
    x.k = (size_t)slot * a.g.n + x.v;
    return x;
}

__global__ void __launch_bounds__(BFS_BLOCK) k_bfs_claim(BfsArgs a) {
    const bfs_u64 E = a.tot[0], stride = (bfs_u64)gridDim.x * blockDim.x;
    for (bfs_u64 e = (bfs_u64)blockIdx.x * blockDim.x + threadIdx.x; e < E; e += stride) {
        const BfsEdge x = bfs_edge(a, e);
        const unsigned k = a.key[x.k]; // (a stale value is only ever larger: at worst an atomic that changes nothing)
        if (k != 0 && k > x.claim)
            atomicMin(&a.key[x.k], x.claim);
    }
}

// the contiguous edge range of workgroup b: [b * per, min(E, (b + 1) * per)), per a multiple of the workgroup's width
DEVI void bfs_range(bfs_u64 E, bfs_u64 &e0, bfs_u64 &e1) {
    bfs_u64 per = (E + gridDim.x - 1) / gridDim.x;
    per = (per + BFS_BLOCK - 1) / BFS_BLOCK * BFS_BLOCK;
    e0 = (bfs_u64)blockIdx.x * per < E ? (bfs_u64)blockIdx.x * per : E;
    e1 = e0 + per < E ? e0 + per : E;
}

__global__ void __launch_bounds__(BFS_BLOCK) k_bfs_count(BfsArgs a) {
    bfs_u64 e0, e1;
    bfs_range(a.tot[0], e0, e1);
    unsigned wins = 0;
    for (bfs_u64 base = e0; base < e1; base += BFS_BLOCK) { // (base and e1 are the same in every lane)
        const bfs_u64 e = base + threadIdx.x;
        int won = 0;
        if (e < e1) {
            const BfsEdge x = bfs_edge(a, e);
            won = a.key[x.k] == x.claim;
        }
        wins += (unsigned)__syncthreads_count(won);
    }
    if (threadIdx.x == 0) {
        a.range_cnt[blockIdx.x] = wins;
        if (wins)
            atomicAdd(&a.tot[1], (bfs_u64)wins); // (an integer sum: the order of the additions does not enter it)
    }
}

__global__ void __launch_bounds__(BFS_BLOCK) k_bfs_emit(BfsArgs a) {
    __shared__ bfs_u64 part[BFS_BLOCK];
    __shared__ int wsum[BFS_BLOCK / 64];
    bfs_u64 e0, e1;
    bfs_range(a.tot[0], e0, e1);
    bfs_u64 mine = 0; // wins of the ranges before this one
    for (unsigned b = threadIdx.x; b < blockIdx.x; b += BFS_BLOCK)
        mine += a.range_cnt[b];
    part[threadIdx.x] = mine;
    __syncthreads();
    for (int s = BFS_BLOCK / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s)
            part[threadIdx.x] += part[threadIdx.x + s];
        __syncthreads();
    }
    bfs_u64 pos0 = part[0];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    for (bfs_u64 base = e0; base < e1; base += BFS_BLOCK) {
        const bfs_u64 e = base + threadIdx.x;
        BfsEdge x = {};
        int won = 0;
        if (e < e1) {
            x = bfs_edge(a, e);
            won = a.key[x.k] == x.claim;
        }
        const bfs_u64 ballot = __ballot(won);
        const int in_wave = __popcll(ballot & (((bfs_u64)1 << lane) - 1));
        if (lane == 0)
            wsum[wv] = __popcll(ballot);
        __syncthreads();
        int before = 0, total = 0;
        for (int k = 0; k < BFS_BLOCK / 64; k++) {
            if (k < wv)
                before += wsum[k];
            total += wsum[k];
        }
        __syncthreads();
        if (won) {
            const long long q = a.f0 + a.F + (long long)(pos0 + before + in_wave);
            a.p_node[q] = x.v;
            a.p_parent[q] = x.u;
            a.p_slot[q] = (int)(x.k / (size_t)a.g.n);
            a.p_depth[q] = a.depth;
            a.key[x.k] = 0;
        }
        pos0 += total;
    }
}

__global__ void __launch_bounds__(BFS_BLOCK) k_bfs_reset(long long used, int n, const int *p_node, const int *p_slot, unsigned *key) {
    const long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (q < used)
        key[(size_t)p_slot[q] * n + p_node[q]] = BFS_UNTOUCHED;
}

__global__ void __launch_bounds__(BFS_BLOCK) k_bfs_iota(long long used, unsigned *idx) {
    const long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (q < used)
        idx[q] = (unsigned)q;
}

// the pool in seed-major order: row r is pool entry order[r]; a seed's rows start where its slot first appears
__global__ void __launch_bounds__(BFS_BLOCK) k_bfs_gather(long long used, const unsigned *order, const int *slot_sorted, const int *p_node,
                                                          const int *p_depth, const int *p_parent, int *o_node, int *o_depth,
                                                          int *o_parent, long long *rowoff) {
    const long long r = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= used)
        return;
    const unsigned q = order[r];
    o_node[r] = p_node[q];
    o_depth[r] = p_depth[q];
    o_parent[r] = p_parent[q];
    if (r == 0 || slot_sorted[r - 1] != slot_sorted[r])
        rowoff[slot_sorted[r]] = r;
}

// ───────────────────────── host ─────────────────────────

#define BFS_WHO "mn_graph_bfs"

// the pool's four columns to `need` entries (twice what it had, if that is more), the first `keep` kept.  A column that
// fails leaves the others grown: pool_cap() is the smallest of the four, and the next call takes them on from where they are.
static int bfs_pool_fit(BfsWork *w, size_t need, size_t keep, hipStream_t st) {
    if (need <= w->pool_cap())
        return 0;
    const size_t ncap = std::max(need, w->pool_cap() * 2);
    for (DevBuf<int> *col : {&w->p_node, &w->p_parent, &w->p_slot, &w->p_depth})
        if (col->grow(gset_err, BFS_WHO, ncap, keep, st))
            return -1;
    return 0;
}

extern "C" int64_t mn_graph_bfs(mn_graph *g, int direction, int64_t n_seeds, const int *seeds, int max_depth, int64_t *row_off,
                                mn_bfs_stats *stats) try {
    GCHK(hipSetDevice(g->device));
    const int N = g->n;
    if (stats)
        memset(stats, 0, sizeof(*stats));
    if (g->bfs)
        g->bfs->rows.valid = false;
    int use_out, use_in;
    if (trav_check_args(BFS_WHO, g, direction, n_seeds, seeds, row_off, &use_out, &use_in))
        return -1;
    if ((bfs_u64)g->e_out + (bfs_u64)g->e_in > 0xFFFFFFFFull - 2) { // e_local + 1 must stay below the "untouched" word
        gset_err("mn_graph_bfs: more than 2^32 - 3 list entries");
        return -1;
    }
    if (trav_check_seeds(BFS_WHO, g, direction, n_seeds, seeds))
        return -1;
    if (!g->bfs)
        g->bfs = new BfsWork();
    BfsWork *w = g->bfs;
    w->rows.clear();
    g->last_ms = 0;
    if (n_seeds == 0 || max_depth <= 0) { // no launch: the start rows and nothing else (:282)
        w->rows.seeds_only(n_seeds, seeds, row_off);
        if (stats)
            stats->rows = n_seeds;
        return n_seeds;
    }
    hipStream_t st = g->stream;
    const size_t per_slot = BFS_BYTES_PER_NODE_SLOT * (size_t)N;
    const size_t S = scratch_chunk((size_t)n_seeds, scratch_budget("MN_BFS_SCRATCH_MB", 0), per_slot, (size_t)0x7fffffff / (size_t)N);
    if (w->key.cap < S * (size_t)N) {
        w->key_clean = false;
        if (w->key.fit(gset_err, BFS_WHO, S * (size_t)N)) {
            gset_err("mn_graph_bfs: out of device memory (N = %d, %zu seeds at once)", N, S);
            return -1;
        }
    }
    if (w->seg_e.fit(gset_err, BFS_WHO, S) || w->d_seeds.fit(gset_err, BFS_WHO, S) || w->d_rowoff.fit(gset_err, BFS_WHO, S))
        return -1;
    if (w->range_cnt.fit(gset_err, BFS_WHO, BFS_MAX_RANGES) || w->tot.fit(gset_err, BFS_WHO, 4)) {
        gset_err("mn_graph_bfs: out of device memory");
        return -1;
    }
    if (bfs_pool_fit(w, std::min<size_t>(S * (size_t)N, std::max<size_t>(S * 64, (size_t)1 << 20)), 0, st))
        return -1;
    if (!w->key_clean) {
        GCHK(hipMemsetAsync(w->key, 0xFF, w->key.cap * sizeof(unsigned), st));
        w->key_clean = true;
    }
    const int max_deg = use_in ? g->max_deg_both : g->max_deg_out; // (out + in bounds the in-lists alone too)
    const BfsDegOf deg_of = {g->off_out, g->off_in, use_out, use_in};
    int64_t rows = 0, levels = 0, chunks = 0, edges = 0;
    double device_ms = 0;
    std::vector<long long> h_rowoff;
    for (int64_t s0 = 0; s0 < n_seeds; s0 += (int64_t)S) {
        const int Sc = (int)std::min<int64_t>((int64_t)S, n_seeds - s0);
        chunks++;
        w->key_clean = false; // until this chunk's entries have been reset
        BfsArgs a;
        memset(&a, 0, sizeof(a));
        a.g = dev_graph_of(g);
        a.use_out = use_out;
        a.use_in = use_in;
        a.key = w->key;
        a.seg_e = w->seg_e;
        a.range_cnt = w->range_cnt;
        a.tot = w->tot;
        GCHK(hipMemcpyAsync(w->d_seeds, seeds + s0, (size_t)Sc * sizeof(int), hipMemcpyHostToDevice, st));
        GCHK(hipEventRecord(g->ev0, st));
        hipLaunchKernelGGL(k_bfs_seed, dim3((Sc + BFS_BLOCK - 1) / BFS_BLOCK), dim3(BFS_BLOCK), 0, st, Sc, N, w->d_seeds, w->key,
                           w->p_node, w->p_parent, w->p_slot, w->p_depth, w->tot);
        long long f0 = 0, F = Sc; // the frontier: pool[f0 .. f0 + F)
        bfs_u64 h_tot[3] = {0, 0, 0};
        for (int depth = 1; depth <= max_depth && F > 0; depth++) {
            if ((size_t)F > w->iscan.cap && w->iscan.fit(gset_err, BFS_WHO, std::max((size_t)F, w->iscan.cap + w->iscan.cap / 2)))
                return -1;
            a.p_node = w->p_node;
            a.p_parent = w->p_parent;
            a.p_slot = w->p_slot;
            a.p_depth = w->p_depth;
            a.f0 = f0;
            a.F = F;
            a.iscan = w->iscan;
            a.depth = depth;
            auto degs = rocprim::make_transform_iterator(w->p_node.p + f0, deg_of);
            if (prim_run(BFS_WHO, "rocprim::inclusive_scan", w->tmp, st, [&](void *tmp, size_t &bytes) {
                    return rocprim::inclusive_scan(tmp, bytes, degs, w->iscan.p, (size_t)F, rocprim::plus<bfs_u64>(), st);
                }))
                return -1;
            hipLaunchKernelGGL(k_bfs_segments, dim3(launch_blocks((bfs_u64)F, BFS_BLOCK, 0x7fffffffu)), dim3(BFS_BLOCK), 0, st, a, w->seg_e);
            const bfs_u64 e_bound = (bfs_u64)F * (bfs_u64)std::max(1, max_deg);
            hipLaunchKernelGGL(k_bfs_claim, dim3(launch_blocks(e_bound, BFS_BLOCK, 8192)), dim3(BFS_BLOCK), 0, st, a);
            const unsigned ranges = launch_blocks(e_bound, BFS_BLOCK * 8, BFS_MAX_RANGES);
            hipLaunchKernelGGL(k_bfs_count, dim3(ranges), dim3(BFS_BLOCK), 0, st, a);
            if (graph_mark(g))
                return -1;
            GCHK(hipMemcpyAsync(h_tot, w->tot, sizeof(h_tot), hipMemcpyDeviceToHost, st)); // the level's one round trip
            if (graph_wait(g, &device_ms))
                return -1;
            levels++;
            const long long W = (long long)h_tot[1];
            if (bfs_pool_fit(w, (size_t)(f0 + F + W), (size_t)(f0 + F), st))
                return -1;
            a.p_node = w->p_node;
            a.p_parent = w->p_parent;
            a.p_slot = w->p_slot;
            a.p_depth = w->p_depth;
            GCHK(hipEventRecord(g->ev0, st));
            if (W > 0)
                hipLaunchKernelGGL(k_bfs_emit, dim3(ranges), dim3(BFS_BLOCK), 0, st, a);
            f0 += F;
            F = W;
        }
        const long long used = f0 + F;
        edges += (int64_t)h_tot[2];
        // seed-major rows: a stable sort of the pool by slot, then one gather
        DevArena scr;
        int *slot_sorted = scr.alloc<int>((size_t)used);
        unsigned *idx = scr.alloc<unsigned>((size_t)used), *order = scr.alloc<unsigned>((size_t)used);
        int *o_node = scr.alloc<int>((size_t)used), *o_depth = scr.alloc<int>((size_t)used), *o_parent = scr.alloc<int>((size_t)used);
        int bits = 1;
        while (bits < 31 && ((long long)1 << bits) < Sc)
            bits++;
        if (!slot_sorted || !idx || !order || !o_node || !o_depth || !o_parent) {
            gset_err("mn_graph_bfs: out of device memory (%lld rows in one chunk)", used);
            return -1;
        }
        const dim3 grid_u(launch_blocks((bfs_u64)used, BFS_BLOCK, 0x7fffffffu));
        hipLaunchKernelGGL(k_bfs_iota, grid_u, dim3(BFS_BLOCK), 0, st, used, idx);
        if (prim_run(BFS_WHO, "rocprim::radix_sort_pairs", w->tmp, st, [&](void *tmp, size_t &bytes) {
                return rocprim::radix_sort_pairs(tmp, bytes, w->p_slot.p, slot_sorted, idx, order, (size_t)used, 0, bits, st);
            }))
            return -1;
        hipLaunchKernelGGL(k_bfs_gather, grid_u, dim3(BFS_BLOCK), 0, st, used, order, slot_sorted, w->p_node, w->p_depth, w->p_parent,
                           o_node, o_depth, o_parent, w->d_rowoff);
        hipLaunchKernelGGL(k_bfs_reset, grid_u, dim3(BFS_BLOCK), 0, st, used, N, w->p_node, w->p_slot, w->key);
        if (graph_mark(g) || w->rows.append(st, (size_t)used, o_node, o_depth, o_parent))
            return -1;
        h_rowoff.resize((size_t)Sc);
        GCHK(hipMemcpyAsync(h_rowoff.data(), w->d_rowoff, (size_t)Sc * sizeof(long long), hipMemcpyDeviceToHost, st));
        if (graph_wait(g, &device_ms))
            return -1;
        w->key_clean = true;
        for (int s = 0; s < Sc; s++)
            row_off[s0 + s] = rows + h_rowoff[(size_t)s];
        rows += used;
    }
    row_off[n_seeds] = rows;
    g->last_ms = device_ms;
    if (stats) {
        stats->rows = rows;
        stats->levels = levels;
        stats->chunks = chunks;
        stats->edges_scanned = edges;
        stats->device_ms = device_ms;
    }
    w->rows.valid = true;
    return rows;
} MN_GUARD_END(gset_err, MN_NOTHING, -1)

extern "C" int mn_graph_bfs_rows(mn_graph *g, int *node, int *depth, int *parent) try {
    return trav_rows_out(g->bfs ? &g->bfs->rows : nullptr, BFS_WHO, node, depth, parent);
} MN_GUARD_END(gset_err, MN_NOTHING, -1)
