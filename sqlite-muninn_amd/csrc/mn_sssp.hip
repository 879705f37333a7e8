// mn_sssp.hip — shortest paths over an mn_graph's device-resident out-lists, gfx950:
//   mn_graph_shortest_paths        graph_shortest_path (src/graph_tvf.c:472-753) for many (start, end) pairs at once
//   mn_graph_shortest_paths_rows   the (node, distance) rows of the last call
//
// Three procedures behind the one entry point:
//
//   replay      k_sp_replay: run_shortest_path_dijkstra (:600-753) as it is written, one wavefront per pair.  The reference's
//               "priority queue" is an array: the pop is a linear scan for the first index of the strict minimum (:646-650), the
//               last entry moves into the hole (:652), a popped entry whose node is settled is dropped (:655), and every list
//               entry of a newly settled node whose target is not settled is appended in list order (:681-696).  The scan is a
//               64-lane reduction on (dist, index), the append a ballot and a prefix count; ties, stale pops, negative and
//               infinite weights come out as the reference's because the array holds the same entries at the same indices.
//
//   fast        k_sssp_*: a label-correcting SSSP per distinct start, several starts to a launch.  dist is the u64 bit pattern
//               of a non-negative f64 (which orders as the value does; all ones = not reached, above +inf), a relaxation is one
//               64-bit atomicMin, a lowered node enters the next frontier if its new label is within the start's threshold and
//               is marked pending otherwise.  When the frontier runs dry the threshold moves to (least pending label) + delta;
//               a start whose least pending label exceeds the largest label of its ends is done.  With weights >= 0,
//               fl(a + w) is monotone in a and never below a, so the fixpoint is what the reference's Dijkstra settles, bit
//               for bit, under any schedule.  Parents are a second pass, k_tight_level: a level-synchronous BFS from the start
//               over TIGHT edges (fl(dist[u] + w) == dist[v]); a node's parent is the tight edge from the previous level with
//               the smallest number in the forward lists, one atomicMin on (level << 32 | list entry).  In words: fewest
//               edges among the shortest paths, then the lowest (parent index, place in its list).  Nothing of this depends on
//               delta, on the launch shape or on how starts are chunked.
//
//   unweighted  run_shortest_path_bfs (:472-586): first-discovery parents are what mn_graph_bfs's rows hold; one traversal per
//               distinct start, traced back on the host side of this file.
#include "mn_graph_int.hpp"
#include "mn_guard.hpp"

#include <climits>
#include <cmath>
#include <cstring>
#include <numeric>

typedef unsigned long long sp_u64;

#define SP_WAVE 64
#define SP_BLOCK 256
#define SP_UNSETTLED (-1) // replay's parent word before a node is settled (a byte fill of 0xFF)
#define SP_NONE (-2)      // the start's parent
#define SP_NOT_REACHED 0xFFFFFFFFFFFFFFFFull
#define SP_KEY_UNSET 0xFFFFFFFFFFFFFFFFull
#define SP_FAR 0xFFFFFFFFu // fast mode's stamp of a node that was lowered beyond the threshold and waits
#define SP_REPLAY_BYTES_PER_ENTRY ((size_t)16)
#define SP_REPLAY_BYTES_PER_NODE ((size_t)12)
#define SP_FAST_BYTES_PER_NODE_SLOT ((size_t)40) // dist 8, key 8, stamp 4, two frontiers of 8 each, rounded up

struct SpWork {
    bool scanned = false; // the weights were looked at (a handle's lists never change)
    long long n_neg = 0, n_nan = 0, n_ninf = 0;
    double mean_w = 0;
    std::vector<int> r_node;
    std::vector<double> r_dist;
    bool rows_valid = false;
};

void sp_work_free(SpWork *w) { delete w; }

// ───────────────────────── the weights, once per handle ─────────────────────────

// out[0] negative, out[1] NaN, out[2] -inf, out[3] finite weights counted; *sum their sum (tuning only: delta's default)
__global__ void __launch_bounds__(SP_BLOCK) k_sp_wscan(long long E, const double *w, sp_u64 *out, double *sum) {
    long long neg = 0, nan = 0, ninf = 0, fin = 0;
    double s = 0;
    for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < E; e += (long long)gridDim.x * blockDim.x) {
        const double x = w[e];
        if (x != x)
            nan++;
        else if (x < 0) {
            neg++;
            if (isinf(x))
                ninf++;
        }
        if (isfinite(x)) {
            fin++;
            s += x;
        }
    }
    if (neg) atomicAdd(&out[0], (sp_u64)neg);
    if (nan) atomicAdd(&out[1], (sp_u64)nan);
    if (ninf) atomicAdd(&out[2], (sp_u64)ninf);
    if (fin) {
        atomicAdd(&out[3], (sp_u64)fin);
        atomicAdd(sum, s);
    }
}

// ───────────────────────── replay ─────────────────────────

struct ReplayArgs {
    DevGraph g;
    long long Q;          // queue entries per pair: E_out + 1
    double *q_dist;       // [P][Q]
    int *q_node, *q_par;  // [P][Q]
    double *s_dist;       // [P][n] settled distance
    int *s_par;           // [P][n] SP_UNSETTLED, SP_NONE or the parent
    const int *start, *end;
    int *cnt;             // [P] rows of the pair's path, 0 = none
    int *flags;           // [0] a queue would have overflowed, [1] a distance came out NaN
    sp_u64 *ctr;          // [0] pops, [1] pushes
};

__global__ void __launch_bounds__(SP_WAVE) k_sp_replay(ReplayArgs a) {
    const int p = blockIdx.x, lane = threadIdx.x, n = a.g.n;
    double *qd = a.q_dist + (size_t)p * (size_t)a.Q;
    int *qn = a.q_node + (size_t)p * (size_t)a.Q, *qp = a.q_par + (size_t)p * (size_t)a.Q;
    double *sd = a.s_dist + (size_t)p * n;
    int *sp = a.s_par + (size_t)p * n;
    const int start = a.start[p], end = a.end[p];
    if (lane == 0) { // the seed (:637-640)
        qd[0] = 0.0;
        qn[0] = start;
        qp[0] = SP_NONE;
    }
    __syncthreads();
    long long qs = 1, pops = 0, pushes = 0;
    int found = 0, bad = 0;
    while (qs > 0) {
        // the first index of the strict minimum (:646-650): each lane keeps the first of its own stride, the reduction the
        // lower index among equals
        double bd = 0;
        long long bi = -1;
#pragma unroll 4
        for (long long i = lane; i < qs; i += SP_WAVE) {
            const double d = qd[i];
            if (bi < 0 || d < bd) {
                bd = d;
                bi = i;
            }
        }
        for (int o = SP_WAVE / 2; o > 0; o >>= 1) {
            const double od = __shfl_xor(bd, o);
            const long long oi = __shfl_xor(bi, o);
            if (oi >= 0 && (bi < 0 || od < bd || (od == bd && oi < bi))) {
                bd = od;
                bi = oi;
            }
        }
        const int u = qn[bi], par = qp[bi];
        const double du = qd[bi];
        __syncthreads(); // every lane has read the entry before the last one moves into its place (:652)
        if (lane == 0 && bi != qs - 1) {
            qd[bi] = qd[qs - 1];
            qn[bi] = qn[qs - 1];
            qp[bi] = qp[qs - 1];
        }
        qs--;
        pops++;
        __syncthreads();
        if (sp[u] != SP_UNSETTLED) // a stale entry (:655)
            continue;
        if (lane == 0) {
            sp[u] = par;
            sd[u] = du;
        }
        if (u == end) {
            found = 1;
            break;
        }
        __syncthreads(); // a self-loop's target is settled by now
        const int e0 = a.g.off_out[u], e1 = a.g.off_out[u + 1];
        for (int base = e0; base < e1; base += SP_WAVE) {
            const int e = base + lane;
            int push = 0, v = 0;
            double nd = 0;
            if (e < e1) {
                v = a.g.tgt_out[e];
                nd = du + a.g.w_out[e];
                push = sp[v] == SP_UNSETTLED;
            }
            const sp_u64 ballot = __ballot(push);
            const long long pos = qs + __popcll(ballot & (((sp_u64)1 << lane) - 1));
            if (push) {
                if (pos < a.Q) {
                    qd[pos] = nd;
                    qn[pos] = v;
                    qp[pos] = u;
                } else
                    bad |= 1;
                if (nd != nd)
                    bad |= 2;
            }
            const int c = __popcll(ballot);
            qs += c;
            pushes += c;
        }
        if (__any(bad))
            break;
        __syncthreads();
    }
    __syncthreads();
    if (bad & 1)
        a.flags[0] = 1;
    if (bad & 2)
        a.flags[1] = 1;
    if (lane == 0) {
        int c = 0;
        if (found)
            for (int x = end; x != SP_NONE && c <= n; x = sp[x])
                c++;
        a.cnt[p] = c;
        atomicAdd(&a.ctr[0], (sp_u64)pops);
        atomicAdd(&a.ctr[1], (sp_u64)pushes);
    }
}

__global__ void __launch_bounds__(SP_BLOCK) k_sp_replay_trace(int P, int n, const int *end, const int *cnt, const long long *row0,
                                                              const double *s_dist, const int *s_par, int *o_node, double *o_dist) {
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= P)
        return;
    const double *sd = s_dist + (size_t)p * n;
    const int *sp = s_par + (size_t)p * n;
    int x = end[p];
    for (int i = cnt[p] - 1; i >= 0; i--) { // (:709-733)
        o_node[row0[p] + i] = x;
        o_dist[row0[p] + i] = sd[x];
        x = sp[x];
    }
}

// ───────────────────────── fast ─────────────────────────

struct FastArgs {
    DevGraph g;
    sp_u64 *dist;   // [S][n] bits of the label, SP_NOT_REACHED
    unsigned *stamp; // [S][n] the pass a node is queued for, or SP_FAR
    sp_u64 *key;    // [S][n] (tight level << 32) | forward list entry of the parent, SP_KEY_UNSET
    sp_u64 cap;     // entries a frontier holds: S * n
    const int *start;                 // [S]
    const int *end_off, *end_node;    // a slot's ends: end_node[end_off[s] .. end_off[s + 1])
    sp_u64 *thr, *mpend, *maxend;     // [S] threshold, least pending label, largest label of the slot's ends
    int *active;                      // [S]
    sp_u64 *ctr; // [0] entries of the next frontier, [1] relaxations, [2] a frontier would have overflowed
    double delta;
};

DEVI double sp_f64(sp_u64 b) { return __longlong_as_double((long long)b); }
DEVI sp_u64 sp_bits(double d) { return (sp_u64)__double_as_longlong(d); }

__global__ void __launch_bounds__(SP_BLOCK) k_sssp_init(sp_u64 total, sp_u64 *dist, unsigned *stamp, sp_u64 *key) {
    for (sp_u64 i = (sp_u64)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (sp_u64)gridDim.x * blockDim.x) {
        dist[i] = SP_NOT_REACHED;
        stamp[i] = 0;
        key[i] = SP_KEY_UNSET;
    }
}

__global__ void __launch_bounds__(SP_BLOCK) k_sssp_seed(int S, FastArgs a, sp_u64 *q) {
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= S)
        return;
    const int u = a.start[s];
    const size_t k = (size_t)s * a.g.n + u;
    a.dist[k] = 0; // +0.0
    a.stamp[k] = 1;
    a.thr[s] = sp_bits(a.delta);
    a.active[s] = 1;
    q[s] = ((sp_u64)s << 32) | (unsigned)u;
}

// appends the lanes that raise `push` to the next frontier: one atomicAdd per wavefront
DEVI void sp_push(const FastArgs &a, sp_u64 *next, int push, sp_u64 entry, int lane) {
    const sp_u64 ballot = __ballot(push);
    if (!ballot)
        return;
    sp_u64 base = 0;
    const int leader = __ffsll((long long)ballot) - 1;
    if (lane == leader)
        base = atomicAdd(&a.ctr[0], (sp_u64)__popcll(ballot));
    base = __shfl(base, leader);
    if (push) {
        const sp_u64 pos = base + __popcll(ballot & (((sp_u64)1 << lane) - 1));
        if (pos < a.cap)
            next[pos] = entry;
        else
            a.ctr[2] = 1;
    }
}

// one wavefront per frontier entry: its list across the lanes
__global__ void __launch_bounds__(SP_BLOCK) k_sssp_relax(FastArgs a, const sp_u64 *cur, sp_u64 ncur, sp_u64 *next, unsigned pnext) {
    const int lane = threadIdx.x & 63;
    const sp_u64 waves = (sp_u64)gridDim.x * (SP_BLOCK / SP_WAVE);
    sp_u64 relaxed = 0;
    for (sp_u64 i = (sp_u64)blockIdx.x * (SP_BLOCK / SP_WAVE) + (threadIdx.x >> 6); i < ncur; i += waves) {
        const sp_u64 ent = cur[i];
        const int s = (int)(ent >> 32), u = (int)(ent & 0xFFFFFFFFu);
        const size_t row = (size_t)s * a.g.n;
        const double du = sp_f64(a.dist[row + u]); // (a label lowered after this read re-queues the node)
        const sp_u64 thr = a.thr[s];
        const int e0 = a.g.off_out[u], e1 = a.g.off_out[u + 1];
        relaxed += (sp_u64)(e1 - e0);
        for (int base = e0; base < e1; base += SP_WAVE) {
            const int e = base + lane;
            int push = 0, v = 0;
            if (e < e1) {
                v = a.g.tgt_out[e];
                const sp_u64 nb = sp_bits(du + a.g.w_out[e]);
                if (nb < a.dist[row + v] && nb < atomicMin(&a.dist[row + v], nb)) {
                    if (nb <= thr)
                        push = atomicExch(&a.stamp[row + v], pnext) != pnext;
                    else { // pending; a node already queued stays queued
                        const unsigned st = a.stamp[row + v];
                        if (st != pnext && st != SP_FAR)
                            atomicCAS(&a.stamp[row + v], st, SP_FAR);
                    }
                }
            }
            sp_push(a, next, push, ((sp_u64)s << 32) | (unsigned)v, lane);
        }
    }
    if (lane == 0 && relaxed)
        atomicAdd(&a.ctr[1], relaxed);
}

// largest label among a slot's ends; the pending minimum starts over
__global__ void __launch_bounds__(SP_BLOCK) k_sssp_slot_prep(int S, FastArgs a) {
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= S)
        return;
    sp_u64 m = 0;
    for (int j = a.end_off[s]; j < a.end_off[s + 1]; j++)
        m = max(m, a.dist[(size_t)s * a.g.n + a.end_node[j]]);
    a.maxend[s] = m;
    a.mpend[s] = SP_NOT_REACHED;
}

__global__ void __launch_bounds__(SP_BLOCK) k_sssp_pend_min(sp_u64 total, FastArgs a) {
    for (sp_u64 i = (sp_u64)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (sp_u64)gridDim.x * blockDim.x) {
        if (a.stamp[i] != SP_FAR)
            continue;
        const int s = (int)(i / (sp_u64)a.g.n);
        const sp_u64 d = a.dist[i];
        if (a.active[s] && d < a.mpend[s])
            atomicMin(&a.mpend[s], d);
    }
}

// the next threshold; a slot with nothing pending, or nothing pending that could still lower one of its ends, is done
__global__ void __launch_bounds__(SP_BLOCK) k_sssp_slot_thr(int S, FastArgs a) {
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= S || !a.active[s])
        return;
    const sp_u64 m = a.mpend[s];
    if (m == SP_NOT_REACHED || m > a.maxend[s])
        a.active[s] = 0;
    else
        a.thr[s] = sp_bits(sp_f64(m) + a.delta); // >= m: the least pending node is always taken
}

__global__ void __launch_bounds__(SP_BLOCK) k_sssp_collect(sp_u64 total, FastArgs a, sp_u64 *next, unsigned pnext) {
    const int lane = threadIdx.x & 63;
    const sp_u64 stride = (sp_u64)gridDim.x * blockDim.x;
    const sp_u64 rounds = (total + stride - 1) / stride; // (the same in every lane: sp_push is called by whole wavefronts)
    for (sp_u64 r = 0; r < rounds; r++) {
        const sp_u64 i = r * stride + (sp_u64)blockIdx.x * blockDim.x + threadIdx.x;
        int push = 0;
        sp_u64 ent = 0;
        if (i < total && a.stamp[i] == SP_FAR) {
            const int s = (int)(i / (sp_u64)a.g.n);
            if (a.active[s] && a.dist[i] <= a.thr[s]) {
                a.stamp[i] = pnext;
                push = 1;
                ent = ((sp_u64)s << 32) | (unsigned)(i - (sp_u64)s * a.g.n);
            }
        }
        sp_push(a, next, push, ent, lane);
    }
}

__global__ void __launch_bounds__(SP_BLOCK) k_tight_seed(int S, FastArgs a, sp_u64 *q) {
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= S)
        return;
    const int u = a.start[s];
    a.key[(size_t)s * a.g.n + u] = 0; // level 0
    q[s] = ((sp_u64)s << 32) | (unsigned)u;
}

// level `level` of the BFS over tight edges: its nodes claim their targets for level + 1
__global__ void __launch_bounds__(SP_BLOCK) k_tight_level(FastArgs a, const sp_u64 *cur, sp_u64 ncur, sp_u64 *next, unsigned level) {
    const int lane = threadIdx.x & 63;
    const sp_u64 waves = (sp_u64)gridDim.x * (SP_BLOCK / SP_WAVE);
    for (sp_u64 i = (sp_u64)blockIdx.x * (SP_BLOCK / SP_WAVE) + (threadIdx.x >> 6); i < ncur; i += waves) {
        const sp_u64 ent = cur[i];
        const int s = (int)(ent >> 32), u = (int)(ent & 0xFFFFFFFFu);
        const size_t row = (size_t)s * a.g.n;
        const double du = sp_f64(a.dist[row + u]);
        const sp_u64 maxend = a.maxend[s];
        const int e0 = a.g.off_out[u], e1 = a.g.off_out[u + 1];
        for (int base = e0; base < e1; base += SP_WAVE) {
            const int e = base + lane;
            int push = 0, v = 0;
            if (e < e1) {
                v = a.g.tgt_out[e];
                const sp_u64 dv = a.dist[row + v];
                if (dv <= maxend && sp_bits(du + a.g.w_out[e]) == dv) { // tight, and final (labels above maxend may not be)
                    const sp_u64 claim = ((sp_u64)(level + 1) << 32) | (unsigned)e;
                    if (a.key[row + v] > claim) // (a stale value is only ever larger)
                        push = atomicMin(&a.key[row + v], claim) == SP_KEY_UNSET;
                }
            }
            sp_push(a, next, push, ((sp_u64)s << 32) | (unsigned)v, lane);
        }
    }
}

// rows of a pair's path: its end's tight level + 1, or none
__global__ void __launch_bounds__(SP_BLOCK) k_sp_fast_count(int P, int n, const int *p_slot, const int *p_end, const sp_u64 *key, int *cnt) {
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= P)
        return;
    const sp_u64 k = key[(size_t)p_slot[p] * n + p_end[p]];
    cnt[p] = k == SP_KEY_UNSET ? 0 : (int)(k >> 32) + 1;
}

__global__ void __launch_bounds__(SP_BLOCK) k_sp_fast_trace(int P, DevGraph g, const int *p_slot, const int *p_end, const int *cnt,
                                                            const long long *row0, const sp_u64 *dist, const sp_u64 *key, int *o_node,
                                                            double *o_dist) {
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= P)
        return;
    const size_t row = (size_t)p_slot[p] * g.n;
    int x = p_end[p];
    for (int i = cnt[p] - 1; i >= 0; i--) {
        o_node[row0[p] + i] = x;
        o_dist[row0[p] + i] = sp_f64(dist[row + x]);
        if (i == 0)
            break;
        const int e = (int)(key[row + x] & 0xFFFFFFFFu);
        int lo = 0, hi = g.n - 1; // the node whose list holds entry e: the first u with off_out[u + 1] > e
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (g.off_out[mid + 1] > e)
                hi = mid;
            else
                lo = mid + 1;
        }
        x = lo;
    }
}

// ───────────────────────── host ─────────────────────────

struct SpRun { // what the three procedures share: the rows as they come, and where each pair's stand
    mn_graph *g;
    int64_t n_pairs;
    const int *start, *end;
    std::vector<int> t_node;
    std::vector<double> t_dist;
    std::vector<int64_t> p_pos, p_cnt;
    mn_sp_stats st;
    double ms = 0;
    hipStream_t stream() const { return g->stream; }
};

// ev0 .. ev1 around the launches since the last wait, then the wait, and ev0 again for those that follow
static int sp_wait(SpRun &r) {
    if (graph_mark_wait(r.g, &r.ms))
        return -1;
    GCHK(hipEventRecord(r.g->ev0, r.stream()));
    return 0;
}

static int sp_scan_weights(mn_graph *g, SpWork *w) {
    if (w->scanned)
        return 0;
    DevArena scr;
    sp_u64 *d_out = scr.alloc<sp_u64>(4);
    double *d_sum = scr.alloc<double>(1);
    if (!d_out || !d_sum) {
        gset_err("mn_graph_shortest_paths: out of device memory");
        return -1;
    }
    GCHK(hipMemsetAsync(d_out, 0, 4 * sizeof(sp_u64), g->stream));
    GCHK(hipMemsetAsync(d_sum, 0, sizeof(double), g->stream));
    if (g->e_out > 0)
        hipLaunchKernelGGL(k_sp_wscan, dim3(launch_blocks((sp_u64)g->e_out, SP_BLOCK * 8, 1024)), dim3(SP_BLOCK), 0, g->stream, g->e_out,
                           g->w_out, d_out, d_sum);
    GCHK(hipGetLastError());
    sp_u64 h[4];
    double sum = 0;
    GCHK(hipMemcpyAsync(h, d_out, sizeof(h), hipMemcpyDeviceToHost, g->stream));
    GCHK(hipMemcpyAsync(&sum, d_sum, sizeof(sum), hipMemcpyDeviceToHost, g->stream));
    GCHK(hipStreamSynchronize(g->stream));
    w->n_neg = (long long)h[0];
    w->n_nan = (long long)h[1];
    w->n_ninf = (long long)h[2];
    w->mean_w = h[3] ? sum / (double)h[3] : 0.0;
    w->scanned = true;
    return 0;
}

// a chunk's rows from the device to the run: cnt[P] read, offsets made, `trace` launched with them, rows appended
template <typename Trace>
static int sp_take_rows(SpRun &r, int P, const int *d_cnt, const int64_t *pair_of, int64_t pair0, Trace trace) {
    std::vector<int> h_cnt((size_t)P);
    GCHK(hipMemcpyAsync(h_cnt.data(), d_cnt, (size_t)P * sizeof(int), hipMemcpyDeviceToHost, r.stream()));
    if (sp_wait(r))
        return -1;
    std::vector<long long> h_row0((size_t)P);
    long long rows = 0;
    for (int p = 0; p < P; p++) {
        h_row0[(size_t)p] = rows;
        rows += h_cnt[(size_t)p];
    }
    DevArena scr;
    long long *d_row0 = scr.alloc<long long>((size_t)P);
    int *o_node = scr.alloc<int>((size_t)rows);
    double *o_dist = scr.alloc<double>((size_t)rows);
    if (!d_row0 || !o_node || !o_dist) {
        gset_err("mn_graph_shortest_paths: out of device memory (%lld rows in one chunk)", rows);
        return -1;
    }
    GCHK(hipMemcpyAsync(d_row0, h_row0.data(), (size_t)P * sizeof(long long), hipMemcpyHostToDevice, r.stream()));
    trace(d_row0, o_node, o_dist);
    const size_t at = r.t_node.size();
    r.t_node.resize(at + (size_t)rows);
    r.t_dist.resize(at + (size_t)rows);
    if (rows) {
        GCHK(hipMemcpyAsync(r.t_node.data() + at, o_node, (size_t)rows * sizeof(int), hipMemcpyDeviceToHost, r.stream()));
        GCHK(hipMemcpyAsync(r.t_dist.data() + at, o_dist, (size_t)rows * sizeof(double), hipMemcpyDeviceToHost, r.stream()));
    }
    if (sp_wait(r))
        return -1;
    for (int p = 0; p < P; p++) {
        const int64_t pair = pair_of ? pair_of[p] : pair0 + p;
        r.p_pos[(size_t)pair] = (int64_t)at + h_row0[(size_t)p];
        r.p_cnt[(size_t)pair] = h_cnt[(size_t)p];
    }
    return 0;
}

static int sp_replay(SpRun &r) {
    mn_graph *g = r.g;
    const int N = g->n;
    hipStream_t st = r.stream();
    const size_t Q = (size_t)g->e_out + 1;
    const size_t per_pair = SP_REPLAY_BYTES_PER_ENTRY * Q + SP_REPLAY_BYTES_PER_NODE * (size_t)N;
    const size_t P = scratch_chunk((size_t)r.n_pairs, scratch_budget("MN_SP_SCRATCH_MB", 0), per_pair, (size_t)0x7fffffff);
    DevArena scr;
    ReplayArgs a;
    memset(&a, 0, sizeof(a));
    a.g = dev_graph_of(g);
    a.Q = (long long)Q;
    a.q_dist = scr.alloc<double>(P * Q);
    a.q_node = scr.alloc<int>(P * Q);
    a.q_par = scr.alloc<int>(P * Q);
    a.s_dist = scr.alloc<double>(P * (size_t)N);
    a.s_par = scr.alloc<int>(P * (size_t)N);
    int *d_start = scr.alloc<int>(P), *d_end = scr.alloc<int>(P);
    a.cnt = scr.alloc<int>(P);
    a.flags = scr.alloc<int>(2);
    a.ctr = scr.alloc<sp_u64>(2);
    if (!a.q_dist || !a.q_node || !a.q_par || !a.s_dist || !a.s_par || !d_start || !d_end || !a.cnt || !a.flags || !a.ctr) {
        gset_err("mn_graph_shortest_paths: out of device memory (replay, %zu pairs at once, %zu bytes each)", P, per_pair);
        return -1;
    }
    a.start = d_start;
    a.end = d_end;
    GCHK(hipMemsetAsync(a.flags, 0, 2 * sizeof(int), st));
    GCHK(hipMemsetAsync(a.ctr, 0, 2 * sizeof(sp_u64), st));
    GCHK(hipEventRecord(g->ev0, st));
    for (int64_t p0 = 0; p0 < r.n_pairs; p0 += (int64_t)P) {
        const int Pc = (int)std::min<int64_t>((int64_t)P, r.n_pairs - p0);
        r.st.chunks++;
        GCHK(hipMemcpyAsync(d_start, r.start + p0, (size_t)Pc * sizeof(int), hipMemcpyHostToDevice, st));
        GCHK(hipMemcpyAsync(d_end, r.end + p0, (size_t)Pc * sizeof(int), hipMemcpyHostToDevice, st));
        GCHK(hipMemsetAsync(a.s_par, 0xFF, (size_t)Pc * (size_t)N * sizeof(int), st)); // SP_UNSETTLED
        hipLaunchKernelGGL(k_sp_replay, dim3(Pc), dim3(SP_WAVE), 0, st, a);
        const ReplayArgs &ca = a;
        if (sp_take_rows(r, Pc, a.cnt, nullptr, p0, [&](const long long *row0, int *o_node, double *o_dist) {
                hipLaunchKernelGGL(k_sp_replay_trace, dim3(launch_blocks((sp_u64)Pc, SP_BLOCK, 0x7fffffffu)), dim3(SP_BLOCK), 0, st, Pc, N,
                                   ca.end, ca.cnt, row0, ca.s_dist, ca.s_par, o_node, o_dist);
            }))
            return -1;
    }
    int h_flags[2];
    sp_u64 h_ctr[2];
    GCHK(hipMemcpy(h_flags, a.flags, sizeof(h_flags), hipMemcpyDeviceToHost));
    GCHK(hipMemcpy(h_ctr, a.ctr, sizeof(h_ctr), hipMemcpyDeviceToHost));
    if (h_flags[0]) {
        gset_err("mn_graph_shortest_paths: a replay queue outgrew its %zu entries", Q);
        return -1;
    }
    if (h_flags[1]) {
        gset_err("mn_graph_shortest_paths: a distance came out NaN (an infinite weight met an infinite distance of the other sign)");
        return -1;
    }
    r.st.pops = (int64_t)h_ctr[0];
    r.st.pushes = (int64_t)h_ctr[1];
    r.st.sources = (int)std::min<int64_t>(r.n_pairs, INT_MAX);
    return 0;
}

static double sp_delta(const SpWork *w) {
    double d = w->mean_w > 0 && std::isfinite(w->mean_w) ? w->mean_w : INFINITY;
    if (const char *e = getenv("MN_SSSP_DELTA")) {
        char *endp = nullptr;
        const double x = strtod(e, &endp);
        if (endp != e && x >= 0) // (NaN fails the comparison)
            d = x;
    }
    return d;
}

static int sp_fast(SpRun &r, const SpWork *w) {
    mn_graph *g = r.g;
    const int N = g->n;
    hipStream_t st = r.stream();
    // pairs by distinct start, the starts in ascending order; a slot is one start with all of its ends
    std::vector<int64_t> order((size_t)r.n_pairs);
    std::iota(order.begin(), order.end(), (int64_t)0);
    std::stable_sort(order.begin(), order.end(), [&](int64_t x, int64_t y) { return r.start[x] < r.start[y]; });
    std::vector<int> slot_start, pair_slot((size_t)r.n_pairs), pair_end((size_t)r.n_pairs);
    std::vector<int64_t> slot_first; // index into `order` of a slot's first pair
    for (int64_t i = 0; i < r.n_pairs; i++) {
        if (i == 0 || r.start[order[(size_t)i]] != r.start[order[(size_t)i - 1]]) {
            slot_start.push_back(r.start[order[(size_t)i]]);
            slot_first.push_back(i);
        }
        pair_slot[(size_t)i] = (int)slot_start.size() - 1;
        pair_end[(size_t)i] = r.end[order[(size_t)i]];
    }
    slot_first.push_back(r.n_pairs);
    const size_t D = slot_start.size();
    r.st.sources = (int)D;
    const size_t per_slot = SP_FAST_BYTES_PER_NODE_SLOT * (size_t)N;
    const size_t S = scratch_chunk(D, scratch_budget("MN_SP_SCRATCH_MB", 0), per_slot, (size_t)0x7fffffff / (size_t)N);
    const sp_u64 cap = (sp_u64)S * (sp_u64)N;
    DevArena scr;
    FastArgs a;
    memset(&a, 0, sizeof(a));
    a.g = dev_graph_of(g);
    a.cap = cap;
    a.delta = sp_delta(w);
    a.dist = scr.alloc<sp_u64>(cap);
    a.key = scr.alloc<sp_u64>(cap);
    a.stamp = scr.alloc<unsigned>(cap);
    sp_u64 *qa = scr.alloc<sp_u64>(cap), *qb = scr.alloc<sp_u64>(cap);
    int *d_start = scr.alloc<int>(S), *d_end_off = scr.alloc<int>(S + 1);
    a.thr = scr.alloc<sp_u64>(S);
    a.mpend = scr.alloc<sp_u64>(S);
    a.maxend = scr.alloc<sp_u64>(S);
    a.active = scr.alloc<int>(S);
    a.ctr = scr.alloc<sp_u64>(3);
    if (!a.dist || !a.key || !a.stamp || !qa || !qb || !d_start || !d_end_off || !a.thr || !a.mpend || !a.maxend || !a.active || !a.ctr) {
        gset_err("mn_graph_shortest_paths: out of device memory (fast, %zu starts at once, %zu bytes each)", S, per_slot);
        return -1;
    }
    a.start = d_start;
    a.end_off = d_end_off;
    GCHK(hipMemsetAsync(a.ctr, 0, 3 * sizeof(sp_u64), st));
    GCHK(hipEventRecord(g->ev0, st));
    sp_u64 h_ctr[3] = {0, 0, 0};
    auto read_ctr = [&]() -> int {
        GCHK(hipMemcpyAsync(h_ctr, a.ctr, sizeof(h_ctr), hipMemcpyDeviceToHost, st));
        return sp_wait(r);
    };
    for (size_t s0 = 0; s0 < D; s0 += S) {
        const int Sc = (int)std::min(S, D - s0);
        const int64_t i0 = slot_first[s0], i1 = slot_first[s0 + (size_t)Sc]; // the chunk's pairs: order[i0 .. i1)
        if (i1 - i0 > INT_MAX) {
            gset_err("mn_graph_shortest_paths: more than 2^31 - 1 pairs in one chunk");
            return -1;
        }
        const int Pc = (int)(i1 - i0);
        r.st.chunks++;
        std::vector<int> h_end_off((size_t)Sc + 1), h_slot((size_t)Pc);
        for (int s = 0; s <= Sc; s++)
            h_end_off[(size_t)s] = (int)(slot_first[s0 + (size_t)s] - i0);
        for (int p = 0; p < Pc; p++)
            h_slot[(size_t)p] = pair_slot[(size_t)(i0 + p)] - (int)s0;
        DevArena chunk;
        int *d_pend = chunk.alloc<int>((size_t)Pc), *d_pslot = chunk.alloc<int>((size_t)Pc), *d_cnt = chunk.alloc<int>((size_t)Pc);
        if (!d_pend || !d_pslot || !d_cnt) {
            gset_err("mn_graph_shortest_paths: out of device memory (%d pairs in one chunk)", Pc);
            return -1;
        }
        a.end_node = d_pend;
        GCHK(hipMemcpyAsync(d_start, slot_start.data() + s0, (size_t)Sc * sizeof(int), hipMemcpyHostToDevice, st));
        GCHK(hipMemcpyAsync(d_end_off, h_end_off.data(), ((size_t)Sc + 1) * sizeof(int), hipMemcpyHostToDevice, st));
        GCHK(hipMemcpyAsync(d_pend, pair_end.data() + i0, (size_t)Pc * sizeof(int), hipMemcpyHostToDevice, st));
        GCHK(hipMemcpyAsync(d_pslot, h_slot.data(), (size_t)Pc * sizeof(int), hipMemcpyHostToDevice, st));
        const sp_u64 total = (sp_u64)Sc * (sp_u64)N;
        const dim3 grid_all(launch_blocks(total, SP_BLOCK * 4, 8192)), grid_s(launch_blocks((sp_u64)Sc, SP_BLOCK, 0x7fffffffu)), blk(SP_BLOCK);
        hipLaunchKernelGGL(k_sssp_init, grid_all, blk, 0, st, total, a.dist, a.stamp, a.key);
        hipLaunchKernelGGL(k_sssp_seed, grid_s, blk, 0, st, Sc, a, qa);
        sp_u64 *cur = qa, *next = qb, ncur = (sp_u64)Sc;
        for (unsigned pass = 1; pass < SP_FAR - 1; pass++) {
            GCHK(hipMemsetAsync(a.ctr, 0, sizeof(sp_u64), st));
            hipLaunchKernelGGL(k_sssp_relax, dim3(launch_blocks(ncur, SP_BLOCK / SP_WAVE, 8192)), blk, 0, st, a, cur, ncur, next, pass + 1);
            if (read_ctr())
                return -1;
            r.st.passes++;
            if (h_ctr[0] == 0) { // the frontier ran dry: move every live slot's threshold and take what falls under it
                hipLaunchKernelGGL(k_sssp_slot_prep, grid_s, blk, 0, st, Sc, a);
                hipLaunchKernelGGL(k_sssp_pend_min, grid_all, blk, 0, st, total, a);
                hipLaunchKernelGGL(k_sssp_slot_thr, grid_s, blk, 0, st, Sc, a);
                hipLaunchKernelGGL(k_sssp_collect, grid_all, blk, 0, st, total, a, next, pass + 1);
                if (read_ctr())
                    return -1;
            }
            if (h_ctr[2]) {
                gset_err("mn_graph_shortest_paths: a frontier outgrew its %llu entries", cap);
                return -1;
            }
            if (h_ctr[0] == 0)
                break;
            std::swap(cur, next);
            ncur = h_ctr[0];
        }
        // parents: the BFS over tight edges
        hipLaunchKernelGGL(k_sssp_slot_prep, grid_s, blk, 0, st, Sc, a);
        hipLaunchKernelGGL(k_tight_seed, grid_s, blk, 0, st, Sc, a, qa);
        cur = qa;
        next = qb;
        ncur = (sp_u64)Sc;
        for (unsigned level = 0; level < 0x7FFFFFFEu && ncur > 0; level++) {
            GCHK(hipMemsetAsync(a.ctr, 0, sizeof(sp_u64), st));
            hipLaunchKernelGGL(k_tight_level, dim3(launch_blocks(ncur, SP_BLOCK / SP_WAVE, 8192)), blk, 0, st, a, cur, ncur, next, level);
            if (read_ctr())
                return -1;
            if (h_ctr[2]) {
                gset_err("mn_graph_shortest_paths: a frontier outgrew its %llu entries", cap);
                return -1;
            }
            std::swap(cur, next);
            ncur = h_ctr[0];
        }
        hipLaunchKernelGGL(k_sp_fast_count, dim3(launch_blocks((sp_u64)Pc, SP_BLOCK, 0x7fffffffu)), blk, 0, st, Pc, N, d_pslot, d_pend, a.key, d_cnt);
        const FastArgs &ca = a;
        if (sp_take_rows(r, Pc, d_cnt, order.data() + i0, 0, [&](const long long *row0, int *o_node, double *o_dist) {
                hipLaunchKernelGGL(k_sp_fast_trace, dim3(launch_blocks((sp_u64)Pc, SP_BLOCK, 0x7fffffffu)), blk, 0, st, Pc, ca.g, d_pslot, d_pend,
                                   d_cnt, row0, ca.dist, ca.key, o_node, o_dist);
            }))
            return -1;
        GCHK(hipMemcpy(h_ctr, a.ctr, sizeof(h_ctr), hipMemcpyDeviceToHost));
    }
    r.st.relaxations = (int64_t)h_ctr[1];
    return 0;
}

// run_shortest_path_bfs (:472-586): mn_graph_bfs's first-discovery parents, traced back from each end (:541-572)
static int sp_unweighted(SpRun &r) {
    mn_graph *g = r.g;
    const int N = g->n;
    std::vector<int64_t> order((size_t)r.n_pairs);
    std::iota(order.begin(), order.end(), (int64_t)0);
    std::stable_sort(order.begin(), order.end(), [&](int64_t x, int64_t y) { return r.start[x] < r.start[y]; });
    std::vector<int> starts;
    std::vector<int64_t> first;
    for (int64_t i = 0; i < r.n_pairs; i++)
        if (i == 0 || r.start[order[(size_t)i]] != r.start[order[(size_t)i - 1]]) {
            starts.push_back(r.start[order[(size_t)i]]);
            first.push_back(i);
        }
    first.push_back(r.n_pairs);
    const size_t D = starts.size();
    r.st.sources = (int)D;
    const size_t G = std::max<size_t>(1, ((size_t)1 << 24) / (size_t)std::max(N, 1)); // starts per traversal call: its rows are host memory
    std::vector<int> where((size_t)N, -1), b_node, b_parent, path;
    std::vector<int64_t> row_off;
    for (size_t s0 = 0; s0 < D; s0 += G) {
        const size_t Gc = std::min(G, D - s0);
        row_off.assign(Gc + 1, 0);
        mn_bfs_stats bst;
        const int64_t rows = mn_graph_bfs(g, 1, (int64_t)Gc, starts.data() + s0, INT_MAX, row_off.data(), &bst);
        if (rows < 0)
            return -1;
        b_node.resize((size_t)std::max<int64_t>(rows, 1));
        b_parent.resize((size_t)std::max<int64_t>(rows, 1));
        if (mn_graph_bfs_rows(g, b_node.data(), nullptr, b_parent.data()) != 0)
            return -1;
        r.st.chunks += (int)bst.chunks;
        r.st.passes += bst.levels;
        r.st.relaxations += bst.edges_scanned;
        r.ms += bst.device_ms;
        for (size_t s = 0; s < Gc; s++) {
            for (int64_t q = row_off[s]; q < row_off[s + 1]; q++)
                where[(size_t)b_node[(size_t)q]] = (int)(q - row_off[s]);
            for (int64_t i = first[s0 + s]; i < first[s0 + s + 1]; i++) {
                const int64_t pair = order[(size_t)i];
                path.clear();
                for (int x = r.end[pair]; x >= 0 && where[(size_t)x] >= 0; x = b_parent[(size_t)(row_off[s] + where[(size_t)x])])
                    path.push_back(x);
                r.p_pos[(size_t)pair] = (int64_t)r.t_node.size();
                r.p_cnt[(size_t)pair] = (int64_t)path.size();
                for (size_t k = path.size(); k-- > 0;) {
                    r.t_dist.push_back((double)(path.size() - 1 - k)); // distance = place on the path (:568)
                    r.t_node.push_back(path[k]);
                }
            }
            for (int64_t q = row_off[s]; q < row_off[s + 1]; q++)
                where[(size_t)b_node[(size_t)q]] = -1;
        }
    }
    return 0;
}

extern "C" int64_t mn_graph_shortest_paths(mn_graph *g, int mode, int weighted, int64_t n_pairs, const int *start, const int *end,
                                           int64_t *row_off, mn_sp_stats *stats) try {
    GCHK(hipSetDevice(g->device));
    const int N = g->n;
    if (stats)
        memset(stats, 0, sizeof(*stats));
    if (g->sp)
        g->sp->rows_valid = false;
    if (mode < MN_SP_AUTO || mode > MN_SP_FAST) {
        gset_err("mn_graph_shortest_paths: mode must be 0 (auto), 1 (replay) or 2 (fast)");
        return -1;
    }
    if (n_pairs < 0 || (n_pairs > 0 && (!start || !end)) || !row_off) {
        gset_err("mn_graph_shortest_paths: bad arguments (n_pairs = %lld)", (long long)n_pairs);
        return -1;
    }
    if (N > (1 << 26)) {
        gset_err("mn_graph_shortest_paths: more than 2^26 nodes (N = %d)", N);
        return -1;
    }
    if (g->e_out == 0 && g->e_in > 0) { // as mn_graph_bfs: a graph loaded for the reverse direction has no answer here
        gset_err("mn_graph_shortest_paths: the graph does not hold the out-lists (%lld in entries)", g->e_in);
        return -1;
    }
    for (int64_t i = 0; i < n_pairs; i++)
        if (start[i] < 0 || start[i] >= N || end[i] < 0 || end[i] >= N) {
            gset_err("mn_graph_shortest_paths: pair %lld is (%d, %d), outside 0 .. %d", (long long)i, start[i], end[i], N - 1);
            return -1;
        }
    if (!g->sp)
        g->sp = new SpWork();
    SpWork *w = g->sp;
    w->r_node.clear();
    w->r_dist.clear();
    g->last_ms = 0;
    if (n_pairs == 0) {
        row_off[0] = 0;
        w->rows_valid = true;
        return 0;
    }
    SpRun r;
    r.g = g;
    r.n_pairs = n_pairs;
    r.start = start;
    r.end = end;
    r.p_pos.assign((size_t)n_pairs, 0);
    r.p_cnt.assign((size_t)n_pairs, 0);
    memset(&r.st, 0, sizeof(r.st));
    int rc;
    if (!weighted || !g->w_out) {
        r.st.mode_used = MN_SP_UNWEIGHTED;
        rc = sp_unweighted(r);
    } else {
        if (sp_scan_weights(g, w))
            return -1;
        if (w->n_nan || w->n_ninf) {
            gset_err("mn_graph_shortest_paths: the graph holds %lld NaN and %lld -inf weights", w->n_nan, w->n_ninf);
            return -1;
        }
        if (mode == MN_SP_AUTO) {
            long long replay_max = 4096; // where replay stops being the faster of the two
            if (const char *e = getenv("MN_SP_REPLAY_MAX"))
                replay_max = atoll(e);
            mode = w->n_neg > 0 || g->e_out + 1 <= replay_max ? MN_SP_REPLAY : MN_SP_FAST;
        }
        if (mode == MN_SP_FAST && w->n_neg) {
            gset_err("mn_graph_shortest_paths: fast mode needs weights >= 0 (the graph holds %lld negative ones); replay takes them",
                     w->n_neg);
            return -1;
        }
        r.st.mode_used = mode;
        rc = mode == MN_SP_REPLAY ? sp_replay(r) : sp_fast(r, w);
    }
    if (rc)
        return -1;
    int64_t rows = 0;
    for (int64_t i = 0; i < n_pairs; i++) {
        row_off[i] = rows;
        rows += r.p_cnt[(size_t)i];
    }
    row_off[n_pairs] = rows;
    w->r_node.resize((size_t)rows);
    w->r_dist.resize((size_t)rows);
    for (int64_t i = 0; i < n_pairs; i++)
        if (r.p_cnt[(size_t)i]) {
            memcpy(w->r_node.data() + row_off[i], r.t_node.data() + r.p_pos[(size_t)i], (size_t)r.p_cnt[(size_t)i] * sizeof(int));
            memcpy(w->r_dist.data() + row_off[i], r.t_dist.data() + r.p_pos[(size_t)i], (size_t)r.p_cnt[(size_t)i] * sizeof(double));
        }
    r.st.device_ms = r.ms;
    g->last_ms = r.ms;
    if (stats)
        *stats = r.st;
    w->rows_valid = true;
    return rows;
} MN_GUARD_END(gset_err, MN_NOTHING, -1)

extern "C" int mn_graph_shortest_paths_rows(mn_graph *g, int *node, double *distance) try {
    const SpWork *w = g->sp;
    if (!w || !w->rows_valid) {
        gset_err("mn_graph_shortest_paths_rows: no rows (the last mn_graph_shortest_paths on this graph failed, or there was none)");
        return -1;
    }
    if (!w->r_node.empty()) {
        if (node)
            memcpy(node, w->r_node.data(), w->r_node.size() * sizeof(int));
        if (distance)
            memcpy(distance, w->r_dist.data(), w->r_dist.size() * sizeof(double));
    }
    return 0;
} MN_GUARD_END(gset_err, MN_NOTHING, -1)
