// mn_dfs.hip — depth-first traversal over an mn_graph's device-resident CSR, gfx950:
//   mn_graph_dfs        run_dfs (src/graph_tvf.c:322-416) for many start nodes at once, rows in the reference's pop order
//   mn_graph_dfs_rows   the (node, depth, parent) rows of the last call
//
// The reference keeps a stack of (node, depth, parent) items and a visited set: an item is popped, dropped if its node is
// visited, else marked and emitted, and — while depth < max_depth — every neighbour not visited at that moment is pushed (the
// out-list, then the in-list, each in table-row order), so the LAST-listed neighbour is popped first.  The visited set only
// grows, so an item filtered at push time would also be dropped at pop time: the push-time test changes no row, and the item
// stack can be restated with one FRAME per node being expanded:
//
//   frame = (u, cursor); the frame's index is u's depth; the cursor runs from deg(u) down to 0 over out-list ‖ in-list
//   step:  cursor > 0   v = list(u)[cursor - 1 ...]: visited → nothing; else mark v, emit (v, depth + 1, u), and push
//                        (v, deg(v)) if depth + 1 < max_depth (a node without entries gets no frame: it would be popped at once)
//          cursor == 0  pop
//
// One wavefront per seed slot (k_dfs).  The top frame lives in registers.  A step reads up to 64 entries below the cursor
// (lane l takes entry cursor - 1 - l; under `both` a chunk may straddle the out/in boundary), each lane tests its entry's bit
// in the slot's visited bitmap, and a ballot over (in range and not visited) decides: empty → the cursor drops by the chunk;
// else the lowest set lane holds the next node to visit and the cursor drops to just below it.  The lanes fetch their
// candidates' CSR offsets in the same round trip as the visited words and the chosen lane hands degree and list bases over
// by shuffle, so a visit costs two dependent round trips (list chunk; visited words + offsets).
//
// Visibility of the mark: only this wavefront touches its slot's bitmap, but the lane that marks v and the lane that next
// reads v's word differ (a list may name v twice).  The mark is an agent-scope atomic OR whose RETURNED value is consumed
// before the next visited words are read, and those reads are agent-scope atomic loads: both are served by the L2, no stale
// line of the CU's L1 can answer, and the wait on the return orders them.  A fence per step would also drop the L1's CSR lines.
//
// Every slot counts its steps against (list entries followed) + 2 n + 2; a slot that overruns stops and sets its status word,
// and the host reports an internal error.  No loop spins without that bound.
#include "mn_guard.hpp"
#include "mn_prim.hpp"
#include "mn_traverse.hpp"

#include <rocprim/device/device_scan.hpp>

#include <algorithm>
#include <cstring>

typedef unsigned long long dfs_u64;

#define DFS_WAVE 64
#define DFS_BLOCK 256
// per slot: [0] entries scanned, [1] most frames at once, [2] status (0 ok, 1 step bound overrun, 2 a bit marked twice, 3 more
// rows than nodes, 4 more frames than the slot holds — none of which a correct kernel reaches), [3] steps
#define DFS_INFO 4

struct DfsWork {
    DevBuf<int> slot_rows;      // [slots][3][n]: a slot's node, depth and parent columns
    DevBuf<unsigned> vis;       // [slots][words]: the visited bitmaps
    DevBuf<int2> frames;        // [slots][frames_per]: (u, cursor) of the frames below the top one
    DevBuf<int> d_seeds, cnt;   // [slots], [slots + 1]
    DevBuf<long long> rowoff;   // [slots + 1]
    DevBuf<dfs_u64> info;       // [slots][DFS_INFO]
    DevBuf<char> tmp;           // rocPRIM's
    TravRows rows;              // of the last call
};

void dfs_work_free(DfsWork *w) { delete w; }

// ───────────────────────── kernels ─────────────────────────

struct DfsArgs {
    DevGraph g;
    int use_out, use_in;
    int S;              // slots of this launch
    int max_depth;      // > 0
    size_t words;       // visited words per slot
    size_t frames_per;  // frames per slot
    dfs_u64 step_bound;
    const int *seeds;
    int *rows;
    unsigned *vis;
    int2 *frames;
    int *cnt;
    dfs_u64 *info;
};

DEVI int dfs_bcast(int x, int lane) { return __shfl(x, lane, DFS_WAVE); }

__global__ void __launch_bounds__(DFS_WAVE) k_dfs(DfsArgs a) {
    const int slot = blockIdx.x, lane = threadIdx.x;
    if (slot >= a.S)
        return;
    const int n = a.g.n;
    int *const r_node = a.rows + (size_t)slot * 3 * (size_t)n, *const r_depth = r_node + n, *const r_parent = r_depth + n;
    unsigned *const vis = a.vis + (size_t)slot * a.words;
    int2 *const frames = a.frames + (size_t)slot * a.frames_per;

    // everything below is the same in every lane unless it says otherwise
    int u = a.seeds[slot], top = 0, cnt = 1, maxf = 0;
    int ob = a.use_out ? a.g.off_out[u] : 0, dout = a.use_out ? a.g.off_out[u + 1] - ob : 0;
    int ib = a.use_in ? a.g.off_in[u] : 0, cursor = dout + (a.use_in ? a.g.off_in[u + 1] - ib : 0);
    bool need_off = false, done = cursor == 0;
    dfs_u64 scanned = 0, steps = 0;
    unsigned status = 0;
    unsigned mark_old = 0, mark_bit = 0; // per lane: the bit this lane last marked and the word the atomic returned for it
    if (lane == 0) {
        r_node[0] = u;
        r_depth[0] = 0;
        r_parent[0] = -1;
        mark_bit = 1u << (u & 31);
        mark_old = __hip_atomic_fetch_or(&vis[u >> 5], mark_bit, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    if (!done)
        maxf = 1;
    while (!done) {
        if (++steps > a.step_bound) { // cannot happen: every step takes a list entry or pops a frame
            status = 1;
            break;
        }
        if (cursor == 0) { // pop
            if (top == 0)
                break;
            top--;
            int2 f = make_int2(0, 0);
            if (lane == 0) // (the lane that stored it)
                f = frames[top];
            u = dfs_bcast(f.x, 0);
            cursor = dfs_bcast(f.y, 0);
            need_off = true;
            continue;
        }
        if (need_off) { // the list bases of a frame that came back from memory
            ob = a.use_out ? a.g.off_out[u] : 0;
            dout = a.use_out ? a.g.off_out[u + 1] - ob : 0;
            ib = a.use_in ? a.g.off_in[u] : 0;
            need_off = false;
        }
        // round trip 1: the chunk of entries below the cursor, lane l entry cursor - 1 - l
        const int j = cursor - 1 - lane;
        const bool inr = j >= 0;
        int v = 0;
        if (inr)
            v = j < dout ? a.g.tgt_out[ob + j] : a.g.tgt_in[ib + (j - dout)];
        // the last mark has been performed at the L2 before any word is read again: mark_old is the atomic's return value, first
        // used here (so the atomic's round trip runs beside the chunk's), and the loads below stand behind this branch (the bit
        // found set already would be a node visited twice)
        if (__ballot((mark_old & mark_bit) != 0) != 0) {
            status = 2;
            break;
        }
        // round trip 2: visited word and, speculatively, the candidate's list bounds
        unsigned word = 0xFFFFFFFFu;
        int vo0 = 0, vo1 = 0, vi0 = 0, vi1 = 0;
        if (inr) {
            word = __hip_atomic_load(&vis[v >> 5], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (a.use_out) {
                vo0 = a.g.off_out[v];
                vo1 = a.g.off_out[v + 1];
            }
            if (a.use_in) {
                vi0 = a.g.off_in[v];
                vi1 = a.g.off_in[v + 1];
            }
        }
        const bool fresh = inr && !((word >> (v & 31)) & 1u);
        const dfs_u64 ballot = __ballot(fresh);
        if (ballot == 0) { // the whole chunk is visited
            const int took = cursor < DFS_WAVE ? cursor : DFS_WAVE;
            scanned += (dfs_u64)took;
            cursor -= took;
            continue;
        }
        const int l = __ffsll((long long)ballot) - 1; // the entry nearest the cursor: the one the reference pops first
        scanned += (dfs_u64)(l + 1);
        cursor -= l + 1; // the entries above it are visited and stay so
        const int w = dfs_bcast(v, l), w_ob = dfs_bcast(vo0, l), w_dout = dfs_bcast(vo1 - vo0, l), w_ib = dfs_bcast(vi0, l);
        const int w_deg = w_dout + dfs_bcast(vi1 - vi0, l);
        if (lane == l) {
            mark_bit = 1u << (w & 31);
            mark_old = __hip_atomic_fetch_or(&vis[w >> 5], mark_bit, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        if (cnt < n) { // (a slot has at most n rows: every node is marked once)
            if (lane == 0)
                r_node[cnt] = w;
            if (lane == 1)
                r_depth[cnt] = top + 1;
            if (lane == 2)
                r_parent[cnt] = u;
        } else
            status = 3;
        cnt++;
        if (top + 1 < a.max_depth && w_deg > 0) { // push
            if ((size_t)top >= a.frames_per) { // cannot happen: frames are distinct nodes, fewer than max_depth of them
                status = 4;
                break;
            }
            if (lane == 0)
                frames[top] = make_int2(u, cursor);
            top++;
            u = w;
            cursor = w_deg;
            ob = w_ob;
            dout = w_dout;
            ib = w_ib;
            if (top + 1 > maxf)
                maxf = top + 1;
        }
        if (status)
            break;
    }
    if (lane == 0) {
        a.cnt[slot] = cnt < n ? cnt : n;
        a.info[(size_t)slot * DFS_INFO + 0] = scanned;
        a.info[(size_t)slot * DFS_INFO + 1] = (dfs_u64)maxf;
        a.info[(size_t)slot * DFS_INFO + 2] = status;
        a.info[(size_t)slot * DFS_INFO + 3] = steps;
    }
}

// the slots' row areas → seed-major columns: row r belongs to the slot s with rowoff[s] <= r < rowoff[s + 1] (every slot has
// at least its seed's row); consecutive lanes read and write consecutive rows
__global__ void __launch_bounds__(DFS_BLOCK) k_dfs_rows(int S, int n, long long total, const long long *rowoff, const int *rows,
                                                       int *o_node, int *o_depth, int *o_parent) {
    const long long r = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= total)
        return;
    int lo = 0, hi = S - 1; // last slot whose first row is <= r
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (rowoff[mid] <= r)
            lo = mid;
        else
            hi = mid - 1;
    }
    const int *const base = rows + (size_t)lo * 3 * (size_t)n;
    const size_t i = (size_t)(r - rowoff[lo]);
    o_node[r] = base[i];
    o_depth[r] = base[(size_t)n + i];
    o_parent[r] = base[2 * (size_t)n + i];
}

// ───────────────────────── host ─────────────────────────

#define DFS_WHO "mn_graph_dfs"

extern "C" int64_t mn_graph_dfs(mn_graph *g, int direction, int64_t n_seeds, const int *seeds, int max_depth, int64_t *row_off,
                                mn_dfs_stats *stats) try {
    GCHK(hipSetDevice(g->device));
    const int N = g->n;
    if (stats)
        memset(stats, 0, sizeof(*stats));
    if (g->dfs)
        g->dfs->rows.valid = false;
    int use_out, use_in;
    if (trav_check_args(DFS_WHO, g, direction, n_seeds, seeds, row_off, &use_out, &use_in))
        return -1;
    const dfs_u64 followed = (use_out ? (dfs_u64)g->e_out : 0) + (use_in ? (dfs_u64)g->e_in : 0);
    if (followed >= ((dfs_u64)1 << 31)) { // a cursor is a 32-bit count of a node's entries
        gset_err("mn_graph_dfs: 2^31 or more list entries in the lists this direction follows");
        return -1;
    }
    if (trav_check_seeds(DFS_WHO, g, direction, n_seeds, seeds))
        return -1;
    if (!g->dfs)
        g->dfs = new DfsWork();
    DfsWork *w = g->dfs;
    w->rows.clear();
    g->last_ms = 0;
    if (n_seeds == 0 || max_depth <= 0) { // no launch: the start rows and nothing else (:383)
        w->rows.seeds_only(n_seeds, seeds, row_off);
        if (stats)
            stats->rows = n_seeds;
        return n_seeds;
    }
    hipStream_t st = g->stream;
    const size_t words = ((size_t)N + 31) / 32, frames_per = (size_t)std::min(N, max_depth);
    const size_t per_slot = 12 * (size_t)N + words * 4 + 8 * frames_per;
    const size_t S = scratch_chunk((size_t)n_seeds, scratch_budget("MN_DFS_SCRATCH_MB", 0), per_slot, (size_t)0x7fffffff);
    if (w->slot_rows.fit(gset_err, DFS_WHO, S * 3 * (size_t)N) || w->vis.fit(gset_err, DFS_WHO, S * words) ||
        w->frames.fit(gset_err, DFS_WHO, S * frames_per) || w->d_seeds.fit(gset_err, DFS_WHO, S) ||
        w->cnt.fit(gset_err, DFS_WHO, S + 1) || w->rowoff.fit(gset_err, DFS_WHO, S + 1) || w->info.fit(gset_err, DFS_WHO, S * DFS_INFO))
        return -1;
    int64_t rows = 0, chunks = 0, entries = 0, max_frames = 0;
    double device_ms = 0;
    std::vector<long long> h_rowoff;
    std::vector<dfs_u64> h_info;
    for (int64_t s0 = 0; s0 < n_seeds; s0 += (int64_t)S) {
        const int Sc = (int)std::min<int64_t>((int64_t)S, n_seeds - s0);
        chunks++;
        DfsArgs a;
        memset(&a, 0, sizeof(a));
        a.g = dev_graph_of(g);
        a.use_out = use_out;
        a.use_in = use_in;
        a.S = Sc;
        a.max_depth = max_depth;
        a.words = words;
        a.frames_per = frames_per;
        a.step_bound = followed + 2 * (dfs_u64)N + 2;
        a.seeds = w->d_seeds;
        a.rows = w->slot_rows;
        a.vis = w->vis;
        a.frames = w->frames;
        a.cnt = w->cnt;
        a.info = w->info;
        GCHK(hipMemcpyAsync(w->d_seeds, seeds + s0, (size_t)Sc * sizeof(int), hipMemcpyHostToDevice, st));
        GCHK(hipEventRecord(g->ev0, st));
        GCHK(hipMemsetAsync(w->vis, 0, (size_t)Sc * words * sizeof(unsigned), st));
        GCHK(hipMemsetAsync(w->cnt, 0, ((size_t)Sc + 1) * sizeof(int), st));
        hipLaunchKernelGGL(k_dfs, dim3((unsigned)Sc), dim3(DFS_WAVE), 0, st, a);
        if (prim_run(DFS_WHO, "rocprim::exclusive_scan", w->tmp, st, [&](void *tmp, size_t &bytes) {
                return rocprim::exclusive_scan(tmp, bytes, w->cnt.p, w->rowoff.p, (long long)0, (size_t)Sc + 1, rocprim::plus<long long>(), st);
            }) ||
            graph_mark(g))
            return -1;
        h_rowoff.resize((size_t)Sc + 1);
        h_info.resize((size_t)Sc * DFS_INFO);
        GCHK(hipMemcpyAsync(h_rowoff.data(), w->rowoff, ((size_t)Sc + 1) * sizeof(long long), hipMemcpyDeviceToHost, st));
        GCHK(hipMemcpyAsync(h_info.data(), w->info, (size_t)Sc * DFS_INFO * sizeof(dfs_u64), hipMemcpyDeviceToHost, st));
        if (graph_wait(g, &device_ms))
            return -1;
        for (int s = 0; s < Sc; s++) {
            const dfs_u64 *f = &h_info[(size_t)s * DFS_INFO];
            if (f[2] != 0) {
                gset_err("mn_graph_dfs: internal error: seed %lld stopped with status %llu after %llu steps (bound %llu)",
                         (long long)(s0 + s), f[2], f[3], a.step_bound);
                return -1;
            }
            entries += (int64_t)f[0];
            max_frames = std::max<int64_t>(max_frames, (int64_t)f[1]);
        }
        const long long used = h_rowoff[(size_t)Sc];
        DevArena scr;
        int *o_node = scr.alloc<int>((size_t)used), *o_depth = scr.alloc<int>((size_t)used), *o_parent = scr.alloc<int>((size_t)used);
        if (!o_node || !o_depth || !o_parent) {
            gset_err("mn_graph_dfs: out of device memory (%lld rows in one chunk)", used);
            return -1;
        }
        GCHK(hipEventRecord(g->ev0, st));
        hipLaunchKernelGGL(k_dfs_rows, dim3((unsigned)((used + DFS_BLOCK - 1) / DFS_BLOCK)), dim3(DFS_BLOCK), 0, st, Sc, N, used, w->rowoff,
                           w->slot_rows, o_node, o_depth, o_parent);
        if (graph_mark(g) || w->rows.append(st, (size_t)used, o_node, o_depth, o_parent) || graph_wait(g, &device_ms))
            return -1;
        for (int s = 0; s < Sc; s++)
            row_off[s0 + s] = rows + h_rowoff[(size_t)s];
        rows += used;
    }
    row_off[n_seeds] = rows;
    g->last_ms = device_ms;
    if (stats) {
        stats->rows = rows;
        stats->chunks = chunks;
        stats->entries_scanned = entries;
        stats->max_frames = max_frames;
        stats->device_ms = device_ms;
    }
    w->rows.valid = true;
    return rows;
} MN_GUARD_END(gset_err, MN_NOTHING, -1)

extern "C" int mn_graph_dfs_rows(mn_graph *g, int *node, int *depth, int *parent) try {
    return trav_rows_out(g->dfs ? &g->dfs->rows : nullptr, DFS_WHO, node, depth, parent);
} MN_GUARD_END(gset_err, MN_NOTHING, -1)
