// mn_leiden.hip — Leiden community detection (src/graph_community.c:75-429) over device-resident CSR
// adjacency (src/graph_csr.h:27-34), gfx950: the kernels, their workspace, the bookkeeping between phases, the two phase
// drivers and the three entry points.  What a wavefront does to evaluate one node is mn_leiden_eval.hpp.
//
// The reference sweeps nodes in order and applies every move immediately (:158-228).  Schedules:
//   k_leiden_seq     MN_LEIDEN_SEQUENTIAL: ONE wavefront walks v = 0..N-1 with in-place updates (agent-scope atomics for
//                    label / sum_tot: never a stale L1 line) — community assignment and Q bit-identical to the reference
//   k_leiden_eval    MN_LEIDEN_BATCHED: a range of nodes evaluated in parallel against frozen state — a chain of dependent
//                    gathers per node (offsets → targets → labels → sum_tot), so what it needs is nodes in flight: a wavefront
//                    evaluates 64/SG nodes at once in SG-lane sub-groups, the few nodes with more than LEI_SG_CAP edges take a
//                    whole wavefront each (biglist).  The movers' per-community tallies are folded into it (lei_tally).
//   run_phase_sync   the default: whole-graph sweeps, k_leiden_eval + k_leiden_apply_sync applying EVERY positive-gain mover,
//                    every LEI_PICKLESS-th sweep only towards smaller community ids; divided by node range over the ranks
//                    of a communicator
//   run_phase        rounds of `batch` nodes, k_leiden_eval + k_leiden_win + k_leiden_apply: a mover commits iff it is the
//                    smallest-index mover among the movers touching its old/target community and its moving neighbours →
//                    committed moves are pairwise independent, realise exactly their computed gain (Q strictly increases)
//                    and the result does not depend on execution order.  Also what finishes a synchronous phase that does
//                    not settle.
// Weighted graphs: sum_tot receives a round's additions in the reference's order through k_leiden_ops, a stable radix sort
// and k_leiden_apply_ops (lei_apply_weighted); the apply kernels then only move labels.
// The O(N) bookkeeping between phases (m :344-350, distinct counts :388-403, renumber :317-331, sum_tot rebuild :413-416, the
// per-community accumulation of :128-139) comes twice (LeiBook), on the device and on the host.
// All device buffers are allocated once per graph (LeiWork) and reused by later calls.
#include "mn_leiden_eval.hpp"
#include "mn_guard.hpp"
#include "mn_comm.hpp"
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <cstring>

#define LEI_WPB 4 // wavefronts per k_leiden_eval workgroup (at most; power of two)
#define LEI_GROW 4       // tail rule of the batched schedule: round size factor ...
#define LEI_GROW_DIV 256 // ... once a sweep commits fewer than N / 256 moves
#define LEI_GROW_MAX 64  // (upper bound of the MN_LEIDEN_GROW tuning knob)

// ───────────────────────── kernels ─────────────────────────
__global__ void __launch_bounds__(64) k_leiden_seq(LeiArgs a) {
    __shared__ __align__(16) double lds_w[LEI_CAP];
    __shared__ __align__(16) int lds_c[LEI_CAP];
    __shared__ __align__(16) unsigned char lds_e[LEI_CAP];
    const int lane = threadIdx.x;
    int total = 0, improved = 1, sweeps = 0;
    while (improved && sweeps < a.max_sweeps) { // :154-229
        improved = 0;
        sweeps++;
        for (int v = 0; v < a.g.n; v++) {
            const int old = ld_i<true>(a.label + v);
            int best; // two call sites: LDS staging keeps its address space (a runtime-selected pointer would be FLAT)
            if (node_degree(a, v) <= LEI_CAP)
                best = best_move<true>(a.g, v, a.label, a.sum_tot, a.kdeg, a.m, a.resolution, a.use_both, a.elig_part, lds_c,
                                       lds_w, lds_e, lane);
            else
                best = best_move<true>(a.g, v, a.label, a.sum_tot, a.kdeg, a.m, a.resolution, a.use_both, a.elig_part,
                                       a.scratch_c, a.scratch_w, a.scratch_e, lane);
            if (best != old) { // :220-227
                if (lane == 0) {
                    const double k_v = a.kdeg[v];
                    double so = ld_d<true>(a.sum_tot + old), sb = ld_d<true>(a.sum_tot + best);
                    __hip_atomic_store(a.sum_tot + old, so - k_v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    __hip_atomic_store(a.sum_tot + best, sb + k_v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    __hip_atomic_store(a.label + v, best, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                }
                __builtin_amdgcn_s_waitcnt(0);
                improved = 1;
                total++;
            }
        }
    }
    if (lane == 0) {
        a.out[0] = total;
        a.out[1] = sweeps;
        a.out[2] = improved; // 1 → stopped by max_sweeps, not converged
    }
}

// One launch evaluates a whole round: blocks [0, nsmall) take 64/SG nodes each in SG-lane sub-groups (nodes with more
// than LEI_SG_CAP edges are skipped there), blocks [nsmall, nsmall + big1 - big0) take one such wide node each
// (biglist).  HASH = unweighted graph → best_move_hash; otherwise the list-order f64 sums of best_move_wslots; a wide node
// past lds_cap edges: best_move in global scratch.  Dynamic LDS: max(sub-group area, wide-node area) — sized by the host
// (lei_eval_lds).
template <int SG, bool HASH>
__global__ void __launch_bounds__(64 * LEI_WPB) k_leiden_eval(LeiArgs a, int nsmall, unsigned wave_lds) {
    // LEI_WPB independent wavefronts per workgroup (no workgroup barrier anywhere): a quarter of the workgroups to dispatch
    extern __shared__ __align__(16) unsigned char lei_smem_all[];
    unsigned char *lei_smem = lei_smem_all + (threadIdx.x >> 6) * wave_lds;
    const int vblock = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); // the wavefront's index in the launch
    constexpr int NG = 64 / SG;
    const int lane = threadIdx.x & 63;
    if (vblock < nsmall) {
        const int grp = lane / SG, sl = lane % SG;
        const int v = a.b0 + vblock * NG + grp;
        if (v >= a.b1)
            return;
        double dk = 0.0;
        int best;
        const LeiHead hd = lei_head(a.g, v, a.label, a.kdeg, a.use_both, a.elig_part);
        if (hd.d_out + hd.d_in > LEI_SG_CAP)
            return;
        if (HASH) {
            const int H = 1 << a.sg_log2h;
            int *tk = reinterpret_cast<int *>(lei_smem) + grp * LEI_SG_AREA_OF(a.sg_log2h);
            best = best_move_hash<SG>(a.g, hd, a.label, a.sum_tot, a.m, a.resolution, a.elig_part, tk, tk + H, tk + 2 * H, tk + 3 * H,
                                      a.sg_log2h, lane, sl, &dk, a.pickless);
        } else {
            unsigned char *area = lei_smem + (size_t)grp * lei_wslots_bytes(LEI_SG_CAP, LEI_SG_LOG2H - 1);
            best = best_move_wslots<SG>(a.g, hd, a.label, a.sum_tot, a.m, a.resolution, a.elig_part, area, LEI_SG_CAP, LEI_SG_LOG2H - 1,
                                        lane, sl, &dk, a.pickless);
        }
        if (sl == 0)
            lei_tally(a, v, hd.old, best, dk);
        return;
    }
    const int bi = vblock - nsmall;
    if (bi >= a.big1 - a.big0)
        return;
    const int v = a.biglist[a.big0 + bi];
    const int deg = node_degree(a, v);
    double dk = 0.0;
    int best;
    if (HASH && deg <= a.lds_cap) {
        int *tk = reinterpret_cast<int *>(lei_smem);
        const int H = 1 << a.big_log2h;
        const LeiHead hd = lei_head(a.g, v, a.label, a.kdeg, a.use_both, a.elig_part);
        int lg = 8; // the table is sized to this node (≥ its degree: one entry per edge at most), not to the widest one
        while ((1 << lg) < deg)
            lg++;
        best = best_move_hash<64>(a.g, hd, a.label, a.sum_tot, a.m, a.resolution, a.elig_part, tk, tk + H, tk + 2 * H, tk + 3 * H,
                                  lg, lane, lane, &dk, a.pickless);
    } else if (deg <= a.lds_cap) {
        const LeiHead hd = lei_head(a.g, v, a.label, a.kdeg, a.use_both, a.elig_part);
        best = best_move_wslots<64>(a.g, hd, a.label, a.sum_tot, a.m, a.resolution, a.elig_part, lei_smem, a.lds_cap, a.big_log2h, lane,
                                    lane, &dk, a.pickless);
    } else { // more edges than fit in LDS: global scratch, list-order sums
        const size_t o = (size_t)a.bigoff[a.big0 + bi]; // this node's own region (only nodes past LEI_CAP have one)
        best = best_move<false>(a.g, v, a.label, a.sum_tot, a.kdeg, a.m, a.resolution, a.use_both, a.elig_part, a.scratch_c + o,
                                a.scratch_w + o, a.scratch_e + o, lane, &dk, a.pickless);
    }
    if (lane == 0)
        lei_tally(a, v, a.label[v], best, dk);
}

// movers whose smaller-index neighbours in the round do not move ("free"), gain re-checked in the worst order of
// application; 8 lanes share a node's adjacency scan
__global__ void __launch_bounds__(256) k_leiden_win(LeiArgs a) {
    const int tid = blockIdx.x * blockDim.x + threadIdx.x;
    const int v = a.b0 + (tid >> 3), sl = tid & 7;
    if (v >= a.b1)
        return;
    // (a chain of dependent gathers: everything whose address is known is requested at once)
    const int old = a.label[v], best = a.dec[v - a.b0];
    const int xo0 = a.g.off_out[v], xo1 = a.g.off_out[v + 1];
    const int xi0 = a.use_both ? a.g.off_in[v] : 0, xi1 = a.use_both ? a.g.off_in[v + 1] : 0;
    const double k_v = a.kdeg[v], dkv = a.dk[v - a.b0];
    unsigned char win = 0;
    if (best != old) { // (uniform over the node's 8 lanes)
        const unsigned long long Lq = a.Lq[old], Jq = a.Jq[best];
        const double st_o = a.sum_tot[old], st_b = a.sum_tot[best];
        const int cm_o = a.cmin[old], cm_b = a.cmin[best];
        int blocked = 0;
        // four targets per lane in flight, then their four mover flags: every load is unconditional (clamped index), so the
        // compiler issues them back to back instead of one guarded load + wait per edge
        for (int pass = 0; pass < (a.use_both ? 2 : 1); pass++) {
            const int *tgt = pass ? a.g.tgt_in : a.g.tgt_out;
            const int x1 = pass ? xi1 : xo1;
            for (int x = (pass ? xi0 : xo0) + sl; x < x1; x += 32) {
                int w[4], f[4];
#pragma unroll
                for (int j = 0; j < 4; j++)
                    w[j] = tgt[min(x + 8 * j, x1 - 1)]; // (a repeated last edge changes nothing)
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    const bool inr = w[j] >= a.b0 && w[j] < v;
                    f[j] = a.mv[inr ? w[j] - a.b0 : 0] & (inr ? 1 : 0);
                }
                blocked |= f[0] | f[1] | f[2] | f[3];
            }
        }
        blocked |= __shfl_xor(blocked, 1);
        blocked |= __shfl_xor(blocked, 2);
        blocked |= __shfl_xor(blocked, 4);
        if (!blocked && sl == 0) {
            const unsigned long long q = fx_up(k_v);
            const double Lo = (double)(Lq - q) / LEI_FX, Jc = (double)(Jq - q) / LEI_FX;
            const double gain2 = dkv / a.m + a.resolution * k_v * (st_o - Lo - k_v - st_b - Jc) / (2.0 * a.m * a.m);
            const int strict = cm_o == v && cm_b == v;
            win = (unsigned char)((gain2 > 0.0 ? 1 : 0) | (strict ? 2 : 0));
        }
    }
    if (sl == 0)
        a.win[v - a.b0] = win;
    // "this round has a safe winner" is a flag, not a count: a plain store (thousands of atomics on one address cost a
    // mover-heavy round ≈ 10 ns each, even one per wavefront)
    if (win & 1)
        a.out[1 + a.parity] = 1;
}

// resets the round's tallies and applies its winners
__global__ void __launch_bounds__(256) k_leiden_apply(LeiArgs a) {
    __shared__ int blk_moves;
    const int v = a.b0 + blockIdx.x * blockDim.x + threadIdx.x;
    if (threadIdx.x == 0)
        blk_moves = 0;
    if (blockIdx.x == 0 && threadIdx.x == 0)
        a.out[1 + (a.parity ^ 1)] = 0; // the next round's flag (this round reads the other one)
    __syncthreads();
    int applied = 0;
    if (v < a.b1) {
        const int old = a.label[v], best = a.dec[v - a.b0];
        const unsigned char wbits = a.win[v - a.b0];
        const int safe = a.out[1 + a.parity];
        const double k_v = a.kdeg[v];
        if (best != old) {
            a.cmin[old] = 0x7fffffff;
            a.cmin[best] = 0x7fffffff;
            a.Lq[old] = 0;
            a.Jq[best] = 0;
            const int use_bit = safe > 0 ? 1 : 2;
            if (wbits & use_bit) {
                if (a.apply_on_device) {
                    // unweighted graph: degrees are integers, f64 atomic adds are exact → order-free
                    atomicAdd(a.sum_tot + old, -k_v);
                    atomicAdd(a.sum_tot + best, k_v);
                } // (weighted: sum_tot was brought up to date in the reference's addition order by k_leiden_apply_ops)
                a.label[v] = best;
                applied = 1;
            }
        }
    }
    // the sweep's move count: one atomic per workgroup
    const unsigned long long ba = __ballot(applied);
    if (ba && (threadIdx.x & 63) == __ffsll((long long)ba) - 1)
        atomicAdd(&blk_moves, __popcll(ba));
    __syncthreads();
    if (threadIdx.x == 0 && blk_moves)
        atomicAdd(a.out, blk_moves);
}

// Synchronous sweep: every mover applies.  Unweighted graphs: degrees are integers, the f64 atomic adds are exact and
// order-free.  Weighted graphs: sum_tot was brought up to date in node order by k_leiden_apply_ops, only labels move here.
__global__ void __launch_bounds__(256) k_leiden_apply_sync(LeiArgs a) {
    __shared__ int blk_moves;
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    if (threadIdx.x == 0)
        blk_moves = 0;
    __syncthreads();
    int applied = 0;
    if (v < a.b1) {
        const int old = a.label[v], best = a.dec[v];
        if (best != old) {
            if (a.apply_on_device) {
                const double k_v = a.kdeg[v];
                atomicAdd(a.sum_tot + old, -k_v);
                atomicAdd(a.sum_tot + best, k_v);
            }
            a.label[v] = best;
            applied = 1;
        }
    }
    // (k_leiden_apply's epilogue, written out in both: a helper taking the counter by reference compiles to other instructions)
    const unsigned long long ba = __ballot(applied);
    if (ba && (threadIdx.x & 63) == __ffsll((long long)ba) - 1)
        atomicAdd(&blk_moves, __popcll(ba));
    __syncthreads();
    if (threadIdx.x == 0 && blk_moves)
        atomicAdd(a.out, blk_moves);
}

// Weighted graphs: a round's winners applied on the device in the reference's order.  f64 addition is not associative, so
// sum_tot[c] must receive its additions exactly as the sequential loop makes them: winners in node order, each first
// "sum_tot[old] -= k" then "sum_tot[new] += k" (:220-223).  Operation 2·slot is the subtraction, 2·slot + 1 the addition;
// k_leiden_ops keys them by community (non-winners: key = n), a STABLE radix sort groups a community's operations without
// reordering them, and k_leiden_apply_ops lets the lane that holds a community's first operation replay its run.
__global__ void __launch_bounds__(256) k_leiden_ops(LeiArgs a, int n_nodes, int *keys) {
    const int slot = blockIdx.x * blockDim.x + threadIdx.x;
    if (slot >= a.b1 - a.b0)
        return;
    const int v = a.b0 + slot;
    const int old = a.label[v], best = a.dec[slot]; // (labels are written by k_leiden_apply, after this)
    bool winner = best != old; // synchronous sweep: every mover
    if (!a.sync) {
        const int use_bit = a.out[1 + a.parity] > 0 ? 1 : 2;
        winner = winner && (a.win[slot] & use_bit);
    }
    keys[2 * slot] = winner ? old : n_nodes;
    keys[2 * slot + 1] = winner ? best : n_nodes;
}
__global__ void k_leiden_apply_ops(LeiArgs a, int n_nodes, const int *keys_sorted, const int *ops_sorted, int n_ops) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n_ops)
        return;
    const int c = keys_sorted[j];
    if (c >= n_nodes || (j > 0 && keys_sorted[j - 1] == c))
        return;
    double S = a.sum_tot[c];
    for (int i = j; i < n_ops && keys_sorted[i] == c; i++) {
        const int op = ops_sorted[i];
        const double kv = a.kdeg[a.b0 + (op >> 1)];
        S = (op & 1) ? S + kv : S - kv;
    }
    a.sum_tot[c] = S;
}

// weighted_degree (:95-104) and weight_to_community(v, community[v]) (:75-90), list order, f64
__global__ void k_wdeg(DevGraph g, int use_both, double *kdeg) {
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= g.n)
        return;
    double k = 0.0;
    for (int e = g.off_out[v]; e < g.off_out[v + 1]; e++)
        k += g.w_out ? g.w_out[e] : 1.0;
    if (use_both)
        for (int e = g.off_in[v]; e < g.off_in[v + 1]; e++)
            k += g.w_in ? g.w_in[e] : 1.0;
    kdeg[v] = k;
}

__global__ void k_w2c_self(DevGraph g, int use_both, const int *label, double *out, int v0, int v1) {
    const int v = v0 + blockIdx.x * blockDim.x + threadIdx.x; // nodes [v0, v1): one rank's share of the modularity's per-node terms
    if (v >= v1)
        return;
    const int c = label[v];
    double s = 0.0;
    for (int e = g.off_out[v]; e < g.off_out[v + 1]; e++)
        if (label[g.tgt_out[e]] == c)
            s += g.w_out ? g.w_out[e] : 1.0;
    if (use_both)
        for (int e = g.off_in[v]; e < g.off_in[v + 1]; e++)
            if (label[g.tgt_in[e]] == c)
                s += g.w_in ? g.w_in[e] : 1.0;
    out[v] = s;
}

// the device bookkeeping's (unweighted graphs: all sums are exact integers)
__global__ void k_iota(int *p, int n) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n)
        p[i] = i;
}
__global__ void k_sum_d(const double *x, int n, double *out) { // integer-valued terms: exact in any order
    __shared__ double sh[256];
    double acc = 0.0;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x)
        acc += x[i];
    sh[threadIdx.x] = acc;
    __syncthreads();
    for (int s2 = 128; s2 > 0; s2 >>= 1) {
        if ((int)threadIdx.x < s2)
            sh[threadIdx.x] += sh[threadIdx.x + s2];
        __syncthreads();
    }
    if (threadIdx.x == 0)
        atomicAdd(out, sh[0]);
}
__global__ void k_first_seen(const int *label, int n, int *first) { // first[c] = smallest i with label[i] == c
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n)
        atomicMin(first + label[i], i);
}
__global__ void k_first_flag(const int *label, const int *first, int n, int *flag, int *count) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    int f = 0;
    if (i < n) {
        f = first[label[i]] == i;
        flag[i] = f;
    }
    const unsigned long long b = __ballot(f);
    if (count && (threadIdx.x & 63) == 0 && b)
        atomicAdd(count, __popcll(b));
}
// renumber_communities (:317-331): new id = number of distinct labels first seen before this one's first member
__global__ void k_relabel(int *label, const int *first, const int *rank, int n) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n)
        label[i] = rank[first[label[i]]];
}
__global__ void k_scatter_add(const int *label, const double *val, int n, double *acc) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n)
        atomicAdd(acc + label[i], val[i]);
}

// ───────────────────────── run_leiden workspace (one per graph, reused) ─────────────────────────
template <typename T> struct LeiBuf { // a device array the workspace owns; its contents are undefined after alloc
    T *p = nullptr;
    size_t cap = 0; // entries asked for
    LeiBuf() = default;
    LeiBuf(const LeiBuf &) = delete;
    ~LeiBuf() { (void)hipFree(p); }
    operator T *() const { return p; }
    int alloc(size_t n) { // exactly n entries
        (void)hipFree(p);
        p = nullptr, cap = 0;
        GCHK(hipMalloc(&p, (n ? n : 1) * sizeof(T)));
        cap = n;
        return 0;
    }
    int fit(size_t n) { return p && n <= cap ? 0 : alloc(n); } // at least n entries: what there is, or exactly n
};

struct LeiWork {
    int n = 0, big_mode = -1; // what the per-node arrays and biglist / bigoff were made for: node count, use_both
    LeiBuf<int> label, refined, out, dec, cmin, sc, first, flag, rank, biglist, counts;
    LeiBuf<unsigned char> win, mv, se;
    LeiBuf<double> sum_tot, kdeg, tmp, sw, dk, scal, s_in;
    LeiBuf<unsigned long long> Jq, Lq;
    LeiBuf<long long> bigoff;
    // weighted graphs: the round's operations keyed by community, their stable sort (k_leiden_ops / k_leiden_apply_ops)
    LeiBuf<int> okeys, okeys_s, oiota, oops_s;
    LeiBuf<unsigned char> osort_tmp, scan_tmp; // rocPRIM's
    int osort_bits = 0;
    size_t osort_bytes = 0, scan_bytes = 0, scratch_need = 0; // scratch entries: a region per node with more than LEI_CAP edges
    int *h_out = nullptr;    // pinned: per-sweep move counts read back without stalling the launch queue
    hipEvent_t ev_rd[2] = {nullptr, nullptr};
    std::vector<int> h_big; // nodes with more than LEI_SG_CAP edges (for big_mode = use_both)
    ~LeiWork() {
        (void)hipHostFree(h_out);
        for (hipEvent_t e : ev_rd)
            if (e)
                (void)hipEventDestroy(e);
    }
};

void lei_work_free(LeiWork *w) { delete w; }

// (re)size the workspace for this call; everything is kept for the next one
static int lei_prepare(mn_graph *g, int mode, int batch, int use_both, int max_deg) {
    if (!g->work)
        g->work = new LeiWork();
    LeiWork &w = *g->work;
    if (!w.h_out) {
        GCHK(hipHostMalloc(&w.h_out, 8 * sizeof(int)));
        GCHK(hipEventCreateWithFlags(&w.ev_rd[0], hipEventDisableTiming));
        GCHK(hipEventCreateWithFlags(&w.ev_rd[1], hipEventDisableTiming));
    }
    const int N = g->n;
    const size_t n = (size_t)N;
    hipStream_t st = g->stream;
    if (w.n != N) {
        if (w.label.alloc(n) || w.refined.alloc(n) || w.sum_tot.alloc(n) || w.kdeg.alloc(n) || w.tmp.alloc(n + 64) || w.out.alloc(16) ||
            w.cmin.alloc(n) || w.Jq.alloc(n) || w.Lq.alloc(n) || w.first.alloc(n) || w.flag.alloc(n) || w.rank.alloc(n) ||
            w.counts.alloc(8) || w.scal.alloc(8) || w.s_in.alloc(n))
            return -1;
        size_t bytes = 0;
        if (rocprim::exclusive_scan(nullptr, bytes, w.flag.p, w.rank.p, 0, n, rocprim::plus<int>(), st) != hipSuccess) {
            gset_err("rocprim::exclusive_scan (size query) failed");
            return -1;
        }
        if (w.scan_tmp.alloc(bytes ? bytes : 16))
            return -1;
        w.scan_bytes = bytes;
        w.n = N;
        w.big_mode = -1;
    }
    // every round leaves the tallies clean (k_leiden_apply); a call that failed half-way may not have
    GCHK(hipMemsetAsync(w.cmin, 0x7f, n * sizeof(int), st)); // 0x7f7f7f7f > any node index
    GCHK(hipMemsetAsync(w.Jq, 0, n * sizeof(unsigned long long), st));
    GCHK(hipMemsetAsync(w.Lq, 0, n * sizeof(unsigned long long), st));
    if (w.big_mode != use_both) { // nodes the sub-group evaluation leaves to a wavefront of their own
        w.h_big.clear();
        std::vector<long long> h_off;
        size_t need = 0; // scratch entries: Σ degree (int4-aligned) over the nodes that do not fit in LDS — at most 2E + 4N
        for (int v = 0; v < N; v++) {
            const int d = g->h_off_out[v + 1] - g->h_off_out[v] + (use_both ? g->h_off_in[v + 1] - g->h_off_in[v] : 0);
            if (d > LEI_SG_CAP) {
                w.h_big.push_back(v);
                h_off.push_back((long long)need);
                if (d > LEI_CAP)
                    need += ((size_t)d + 7) & ~(size_t)3;
            }
        }
        w.scratch_need = need;
        if (w.biglist.alloc(w.h_big.size()) || w.bigoff.alloc(w.h_big.size()))
            return -1;
        if (!w.h_big.empty()) {
            GCHK(hipMemcpyAsync(w.biglist, w.h_big.data(), w.h_big.size() * sizeof(int), hipMemcpyHostToDevice, st));
            GCHK(hipMemcpyAsync(w.bigoff, h_off.data(), h_off.size() * sizeof(long long), hipMemcpyHostToDevice, st));
            GCHK(hipStreamSynchronize(st)); // (h_off is a local)
        }
        w.big_mode = use_both;
    }
    const size_t nb = (size_t)batch, n_ops = 2 * nb; // a round's decisions, grown to the largest round asked for so far
    if (mode == MN_LEIDEN_BATCHED && (w.dec.fit(nb + 64) || w.dk.fit(nb) || w.win.fit(nb) || w.mv.fit(nb)))
        return -1;
    if (mode == MN_LEIDEN_BATCHED && g->weighted && n_ops > w.okeys.cap) {
        w.osort_bits = 1;
        while (w.osort_bits < 31 && (1ll << w.osort_bits) <= (long long)N) // keys 0..N (N = "not a winner")
            w.osort_bits++;
        size_t bytes = 0; // (a size query reads none of the arrays)
        if (rocprim::radix_sort_pairs(nullptr, bytes, w.okeys.p, w.okeys_s.p, w.oiota.p, w.oops_s.p, n_ops, 0, w.osort_bits, st) != hipSuccess) {
            gset_err("rocprim::radix_sort_pairs (size query) failed");
            return -1;
        }
        // okeys last: its capacity is what brings a call here, so a failure half-way is made good by the next call
        if (w.osort_tmp.alloc(bytes ? bytes : 16) || w.okeys_s.alloc(n_ops) || w.oiota.alloc(n_ops) || w.oops_s.alloc(n_ops) ||
            w.okeys.alloc(n_ops))
            return -1;
        w.osort_bytes = bytes;
        hipLaunchKernelGGL(k_iota, dim3((unsigned)((n_ops + 255) / 256)), dim3(256), 0, st, w.oiota, (int)n_ops);
    }
    // global scratch for nodes whose edges do not fit in LDS: the sequential kernel reuses one region of max_deg entries,
    // the batched rounds give every such node its own (bigoff) — sized by those nodes' degrees, not by the round
    const size_t want = std::max<size_t>(w.scratch_need, (size_t)max_deg);
    if (max_deg > LEI_CAP && (w.sc.fit(want) || w.sw.fit(want) || w.se.fit(want)))
        return -1;
    return 0;
}

// ───────────────────────── phase drivers ─────────────────────────
// the tail rule's constants; MN_LEIDEN_GROW="factor,divisor" is a tuning knob (the oracle reads ORC_LEI_GROW the same way:
// other values give another — equally valid — schedule, so parity holds only when both sides are set alike)
static void lei_grow_setting(int *grow, int *grow_div) {
    *grow = LEI_GROW;
    *grow_div = LEI_GROW_DIV;
    if (const char *e = getenv("MN_LEIDEN_GROW"))
        sscanf(e, "%d,%d", grow, grow_div);
    *grow = std::min(std::max(*grow, 1), LEI_GROW_MAX);
    *grow_div = std::max(*grow_div, 1);
}

// LDS bytes of one k_leiden_eval wavefront
static size_t lei_eval_lds(int sg, bool hash, int lds_cap, int big_log2h, int sg_log2h) {
    const int ng = 64 / sg;
    const size_t small = hash ? (size_t)ng * LEI_SG_AREA_OF(sg_log2h) * sizeof(int) : (size_t)ng * lei_wslots_bytes(LEI_SG_CAP, LEI_SG_LOG2H - 1);
    // table (3 ints per entry) + occupied-entry list: a counter (16 B) and one 16-bit slot per edge
    const size_t big = hash ? (size_t)3 * ((size_t)1 << big_log2h) * sizeof(int) + 16 + (((size_t)lds_cap * 2 + 15) & ~(size_t)15)
                            : lei_wslots_bytes(lds_cap, big_log2h);
    return small > big ? small : big;
}

// evaluation of the nodes [a.b0, a.b1) (+ the wide nodes a.big0..a.big1 of that range) against the frozen state
static void lei_launch_eval(const LeiArgs &a, int nb, int sg, bool hashed, hipStream_t st) {
    const int nsmall = (nb + (64 / sg) - 1) / (64 / sg);
    const unsigned wlds = (unsigned)((lei_eval_lds(sg, hashed, a.lds_cap, a.big_log2h, a.sg_log2h) + 15) & ~(size_t)15);
    int wpb = LEI_WPB; // (wide nodes with large tables: fewer wavefronts per workgroup, 64 KB of dynamic LDS at most)
    while (wpb > 1 && (size_t)wlds * wpb > 60 * 1024)
        wpb >>= 1;
    const dim3 grid((unsigned)((nsmall + a.big1 - a.big0 + wpb - 1) / wpb)), blk(64 * wpb);
    const size_t lds = (size_t)wlds * wpb;
    if (sg == 32 && hashed)
        hipLaunchKernelGGL((k_leiden_eval<32, true>), grid, blk, lds, st, a, nsmall, wlds);
    else if (sg == 32)
        hipLaunchKernelGGL((k_leiden_eval<32, false>), grid, blk, lds, st, a, nsmall, wlds);
    else if (hashed)
        hipLaunchKernelGGL((k_leiden_eval<16, true>), grid, blk, lds, st, a, nsmall, wlds);
    else
        hipLaunchKernelGGL((k_leiden_eval<16, false>), grid, blk, lds, st, a, nsmall, wlds);
}
static int lei_sub_group(const mn_graph *g, int use_both) {
    int sg = (double)(use_both ? g->e_out + g->e_in : g->e_out) / std::max(1, g->n) > 48.0 ? 32 : 16;
    if (const char *e = getenv("MN_LEIDEN_SG")) // tuning knob: 16 or 32 lanes per node
        sg = atoi(e) == 16 ? 16 : 32;
    return sg;
}

// Weighted graph, the decisions of the nb nodes [a.b0, a.b1) are in: several winners may share a community and f64 addition
// is not associative → the operations are grouped by community with a stable sort and every community replays its own in
// node order.  sum_tot is then up to date; the apply kernel that follows moves the labels.
static int lei_apply_weighted(mn_graph *g, const LeiArgs &a, int nb, hipStream_t st) {
    LeiWork &w = *g->work;
    const int n_ops = 2 * nb;
    hipLaunchKernelGGL(k_leiden_ops, dim3((nb + 255) / 256), dim3(256), 0, st, a, g->n, w.okeys);
    size_t bytes = w.osort_bytes;
    if (rocprim::radix_sort_pairs(w.osort_tmp.p, bytes, w.okeys.p, w.okeys_s.p, w.oiota.p, w.oops_s.p, (size_t)n_ops, 0, w.osort_bits, st) !=
        hipSuccess) {
        gset_err("rocprim::radix_sort_pairs failed");
        return -1;
    }
    hipLaunchKernelGGL(k_leiden_apply_ops, dim3((n_ops + 255) / 256), dim3(256), 0, st, a, g->n, w.okeys_s, w.oops_s, n_ops);
    return 0;
}

// one phase (local moving when elig_part == nullptr, refinement otherwise); returns moves, -1 on error
static long long run_phase(mn_graph *g, LeiArgs a, int mode, int batch, int64_t *sweeps_out) {
    hipStream_t st = g->stream;
    int out[3] = {0, 0, 0};
    if (mode == MN_LEIDEN_SEQUENTIAL) {
        GCHK(hipMemsetAsync(a.out, 0, 3 * sizeof(int), st));
        hipLaunchKernelGGL(k_leiden_seq, dim3(1), dim3(64), 0, st, a);
        GCHK(hipGetLastError());
        GCHK(hipMemcpyAsync(out, a.out, sizeof(out), hipMemcpyDeviceToHost, st));
        GCHK(hipStreamSynchronize(st));
        *sweeps_out += out[1];
        if (out[2]) {
            gset_err("mn_graph_leiden: sweeps did not converge within %d (asymmetric adjacency?)", a.max_sweeps);
            return -1;
        }
        return out[0];
    }
    const std::vector<int> &big = g->work->h_big;
    long long total = 0;
    int improved = 1, sweeps = 0, parity = 0;
    const bool hashed = !g->weighted; // every weight 1.0 → counts (best_move_hash)
    const int sg = lei_sub_group(g, a.use_both);
    int *const out_base = a.out; // two counter blocks of 8 ints ([0] moves, [1..2] "has a safe winner" by round parity): sweep s uses block s & 1
    int pending = -1;            // sweep whose move count is still on its way to the host (device-applied moves only)
    // Tail rule (part of the schedule, restated in oracle/mn_graph_oracle.c batched_phase): once the sweep before the
    // previous one committed fewer than N / LEI_GROW_DIV moves, rounds are LEI_GROW times larger — few movers, few
    // conflicts, and a round's cost is mostly its three launches.  "Before the previous one" because the previous sweep's
    // count is still on its way to the host when this sweep is queued.
    int grow, grow_div;
    lei_grow_setting(&grow, &grow_div);
    const int batch0 = batch;
    long long moves_prev2 = -1; // sweep s-2 (as far as the host has seen it)
    while (improved && sweeps < a.max_sweeps) {
        improved = 0;
        sweeps++;
        batch = batch0;
        if (moves_prev2 >= 0 && moves_prev2 < g->n / grow_div)
            batch = (int)std::min<long long>((long long)batch0 * grow, std::max(batch0, g->n));
        const int blk = sweeps & 1;
        a.out = out_base + 8 * blk;
        GCHK(hipMemsetAsync(a.out, 0, 8 * sizeof(int), st));
        parity = 0;
        size_t bigpos = 0;
        for (int b = 0; b < g->n; b += batch) {
            a.b0 = b;
            a.b1 = b + batch < g->n ? b + batch : g->n;
            a.parity = parity;
            const int nb = a.b1 - a.b0;
            a.big0 = (int)bigpos;
            while (bigpos < big.size() && big[bigpos] < a.b1)
                bigpos++;
            a.big1 = (int)bigpos;
            lei_launch_eval(a, nb, sg, hashed, st);
            hipLaunchKernelGGL(k_leiden_win, dim3((nb * 8 + 255) / 256), dim3(256), 0, st, a);
            if (!a.apply_on_device && lei_apply_weighted(g, a, nb, st))
                return -1;
            hipLaunchKernelGGL(k_leiden_apply, dim3((nb + 255) / 256), dim3(256), 0, st, a); // resets tallies (+ applies)
            parity ^= 1;
        }
        GCHK(hipGetLastError());
        // Moves applied on the device: the count of this sweep travels to pinned memory behind the sweep, and the NEXT sweep
        // is queued before the host looks at the PREVIOUS one — the launch queue never drains.  If that previous sweep
        // moved nothing the state is a fixed point: the sweep just queued moves nothing either and is not counted.
        int *h = g->work->h_out + 4 * blk;
        GCHK(hipMemcpyAsync(h, a.out, sizeof(int), hipMemcpyDeviceToHost, st));
        GCHK(hipEventRecord(g->work->ev_rd[blk], st));
        improved = 1;
        if (pending >= 0) {
            const int pb = pending & 1;
            GCHK(hipEventSynchronize(g->work->ev_rd[pb]));
            const int mv = g->work->h_out[4 * pb];
            if (mv == 0) { // `pending` was the last real sweep; the one queued above is redundant
                sweeps = pending;
                improved = 0;
                pending = -1;
                break;
            }
            total += mv;
            moves_prev2 = mv; // `pending` is the sweep before the one just queued
        }
        pending = sweeps;
    }
    if (pending >= 0) { // stopped by max_sweeps
        GCHK(hipEventSynchronize(g->work->ev_rd[pending & 1]));
        total += g->work->h_out[4 * (pending & 1)];
    }
    a.out = out_base;
    GCHK(hipStreamSynchronize(st));
    *sweeps_out += sweeps;
    return total;
}

// A rank's share of the nodes, [v0, v1): `per` nodes a rank, the last ranks' short or empty; no communicator = one rank
struct LeiRange {
    int world, rank, per, v0, v1;
};
static LeiRange lei_rank_range(const mn_comm *c, int N) {
    const int world = c ? c->world : 1, rank = c ? c->rank : 0, per = (N + world - 1) / world, v0 = std::min(N, rank * per);
    return {world, rank, per, v0, std::min(N, v0 + per)};
}

// Default schedule of MN_LEIDEN_BATCHED since round 4: WHOLE-GRAPH synchronous sweeps (oracle/mn_graph_oracle.c sync_phase is
// the restatement, bit for bit).  A sweep = k_leiden_eval over every node against the state frozen at its start +
// k_leiden_apply_sync applying EVERY positive-gain mover (weighted graphs: sum_tot in node order through the stable sort of
// k_leiden_ops).  Simultaneous moves can swap two nodes for ever, so every `period`-th sweep is "pick-less" (Naim et al., GPU
// Louvain): a node may only move to a community with a smaller id.  The phase ends with the first ordinary sweep that moves
// nothing (= the sequential loop's fixed point); Q is not monotone under simultaneous moves, so after LEI_SYNC_CAP sweeps the
// round schedule (run_phase: safe winners, Q strictly increasing) finishes the phase.  Config 5's graph: 16 + 16 sweeps of two
// launches instead of 856 rounds of three.
#define LEI_PICKLESS 3
#define LEI_SYNC_CAP 48
static int lei_round_default(int N) { return (int)std::min<long long>(16384, std::max<long long>(256, N / 32)); }
static long long run_phase_sync(mn_graph *g, mn_comm *c, LeiArgs a, int period, int64_t *sweeps_out) {
    hipStream_t st = g->stream;
    LeiWork &w = *g->work;
    const int N = g->n;
    const bool hashed = !g->weighted;
    const int sg = lei_sub_group(g, a.use_both);
    int cap = LEI_SYNC_CAP;
    if (const char *e = getenv("MN_LEIDEN_SYNC_CAP")) // tuning knob (the oracle reads ORC_LEI_SYNC_CAP the same way)
        cap = atoi(e);
    // Several GPUs (mn_graph_leiden_shared): every rank holds the graph and the whole state; the evaluation — four fifths of a
    // sweep — is divided by node range, the decisions are all-gathered (N ints per sweep) and every replica applies ALL of them,
    // so every rank walks through the same states as one GPU does and ends with its bits.
    const LeiRange r = lei_rank_range(c, N);
    const int bg0 = (int)(std::lower_bound(w.h_big.begin(), w.h_big.end(), r.v0) - w.h_big.begin());
    const int bg1 = (int)(std::lower_bound(w.h_big.begin(), w.h_big.end(), r.v1) - w.h_big.begin());
    int *const dec_all = a.dec;
    a.sync = 1;
    a.parity = 0;
    long long total = 0;
    int sweeps = 0;
    bool converged = false;
    while (sweeps < cap && sweeps < a.max_sweeps) {
        sweeps++;
        a.pickless = period > 0 && sweeps % period == 0;
        // (table size is a matter of speed only: full-size while most neighbours still carry labels of their own)
        a.sg_log2h = sweeps <= 3 || getenv("MN_LEIDEN_FULL_TABLES") ? LEI_SG_LOG2H : LEI_SG_LOG2H - 1;
        GCHK(hipMemsetAsync(a.out, 0, sizeof(int), st));
        a.b0 = r.v0;
        a.b1 = r.v1;
        a.big0 = bg0;
        a.big1 = bg1;
        a.dec = dec_all + r.v0; // (the evaluation stores decision v at dec[v - b0])
        if (r.v1 > r.v0)
            lei_launch_eval(a, r.v1 - r.v0, sg, hashed, st);
        if (r.world > 1) {
            int failed = -1;
            const int ag = mn_comm_agree(c, hipGetLastError() != hipSuccess ? 1 : 0, st, &failed);
            if (ag != 0) {
                if (ag < 0)
                    gset_err("mn_graph_leiden_shared: %s", mn_comm_last_error_str());
                else
                    gset_err("mn_graph_leiden_shared: rank %d failed; all ranks stop", failed);
                return -1;
            }
            if (mn_comm_allgather_dev(c, dec_all + (size_t)r.rank * r.per, dec_all, (size_t)r.per * sizeof(int), st)) {
                gset_err("mn_graph_leiden_shared: %s", mn_comm_last_error_str());
                return -1;
            }
        }
        a.b0 = 0;
        a.b1 = N;
        a.dec = dec_all;
        if (!a.apply_on_device && lei_apply_weighted(g, a, N, st))
            return -1;
        hipLaunchKernelGGL(k_leiden_apply_sync, dim3((N + 255) / 256), dim3(256), 0, st, a);
        GCHK(hipGetLastError());
        GCHK(hipMemcpyAsync(w.h_out, a.out, sizeof(int), hipMemcpyDeviceToHost, st));
        GCHK(hipStreamSynchronize(st));
        const int mv = w.h_out[0];
        total += mv;
        if (mv == 0 && !a.pickless) {
            converged = true;
            break;
        }
    }
    *sweeps_out += sweeps;
    if (!converged) { // the round schedule finishes the phase (a.dec is dec_all again; run_phase sets every round's range)
        a.sync = 0;
        a.pickless = 0;
        a.sg_log2h = LEI_SG_LOG2H;
        const long long more = run_phase(g, a, MN_LEIDEN_BATCHED, lei_round_default(N), sweeps_out);
        if (more < 0)
            return -1;
        total += more;
    }
    return total;
}

// ───────────────────────── bookkeeping between the phases ─────────────────────────
// The three places where run_leiden touches every node outside a phase, written twice and chosen once per call (LeiBook).
// On the device for unweighted graphs under the parallel schedules: every sum is then a sum of integers below 2^53, exact in
// any order, so atomics give the reference's bits; first-seen renumbering = atomicMin of the first index per label + a prefix
// sum over the first-occurrence flags.  On the host otherwise: f64 addition is not associative, the sums are taken in the
// reference's node order.  The device holds k[i] in kdeg when begin runs, the singletons in label / sum_tot after it
// (leiden_impl), the renumbered partition and its sums after after_refinement.

struct LeiRun { // one call, as its bookkeeping sees it
    mn_graph *g;
    mn_comm *c;
    LeiWork &d;
    DevGraph dg;
    hipStream_t st;
    int N, nbN, use_both;
    double m = 0.0;                  // :344-350
    int K = 0;                       // finish: communities, and their s_in / s_tot of compute_modularity (:128-139)
    std::vector<double> s_in, s_tot;
    std::vector<double> k, sum_tot;  // host bookkeeping: k[i], sum_tot[c] ...
    std::vector<int> community, refined; // ... and the two partitions
};
struct LeiBook {
    int (*begin)(LeiRun &r);            // m, not yet halved (:344-349); the host's copy of k[i]
    int (*after_refinement)(LeiRun &r); // adopt `refined` iff not more communities (:385-408), renumber, rebuild sum_tot (:410-416)
    int (*finish)(LeiRun &r, int *community_out); // renumber (:420); K, s_in, s_tot (:109-127); ends the timed span (ev1)
};

// compute_modularity's per-node terms weight_to_community(i, community[i]) (:131): each rank computes those of its node range
// and the ranges are all-gathered — the modularity partials of several GPUs.  (Gathered per NODE rather than reduced per
// community: the per-community f64 sums are then taken in the reference's node order on every rank, the same bits as one GPU.)
static int lei_w2c_all(const LeiRun &run, const int *label, double *tmp) {
    const LeiRange r = lei_rank_range(run.c, run.N);
    if (r.v1 > r.v0)
        hipLaunchKernelGGL(k_w2c_self, dim3((r.v1 - r.v0 + 255) / 256), dim3(256), 0, run.st, run.dg, run.use_both, label, tmp, r.v0, r.v1);
    if (r.world > 1 && mn_comm_allgather_dev(run.c, tmp + (size_t)r.rank * r.per, tmp, (size_t)r.per * sizeof(double), run.st)) {
        gset_err("mn_graph_leiden_shared: %s", mn_comm_last_error_str());
        return -1;
    }
    return 0;
}

// distinct labels of `label` → counts[slot] (device), leaves first[] / flag[] describing `label`
static int dev_distinct(LeiRun &r, const int *label, int slot) {
    GCHK(hipMemsetAsync(r.d.first, 0x7f, (size_t)r.N * sizeof(int), r.st));
    GCHK(hipMemsetAsync(r.d.counts + slot, 0, sizeof(int), r.st));
    hipLaunchKernelGGL(k_first_seen, dim3(r.nbN), dim3(256), 0, r.st, label, r.N, r.d.first);
    hipLaunchKernelGGL(k_first_flag, dim3(r.nbN), dim3(256), 0, r.st, label, r.d.first, r.N, r.d.flag, r.d.counts + slot);
    return 0;
}
// renumber `label` in place in first-seen order (first[] / flag[] must describe it: dev_distinct)
static int dev_renumber(LeiRun &r, int *label) {
    size_t bytes = r.d.scan_bytes;
    if (rocprim::exclusive_scan(r.d.scan_tmp.p, bytes, r.d.flag.p, r.d.rank.p, 0, (size_t)r.N, rocprim::plus<int>(), r.st) != hipSuccess) {
        gset_err("rocprim::exclusive_scan failed");
        return -1;
    }
    hipLaunchKernelGGL(k_relabel, dim3(r.nbN), dim3(256), 0, r.st, label, r.d.first, r.d.rank, r.N);
    return 0;
}
static int dev_begin(LeiRun &r) {
    GCHK(hipMemsetAsync(r.d.scal, 0, sizeof(double), r.st));
    hipLaunchKernelGGL(k_sum_d, dim3(std::min(r.nbN, 1024)), dim3(256), 0, r.st, r.d.kdeg, r.N, r.d.scal);
    GCHK(hipMemcpyAsync(&r.m, r.d.scal, sizeof(double), hipMemcpyDeviceToHost, r.st));
    GCHK(hipStreamSynchronize(r.st));
    return 0;
}
static int dev_after_refinement(LeiRun &r) {
    LeiWork &d = r.d;
    int cnt[2] = {0, 0};
    if (dev_distinct(r, d.label, 0) || dev_distinct(r, d.refined, 1))
        return -1;
    GCHK(hipMemcpyAsync(cnt, d.counts, sizeof(cnt), hipMemcpyDeviceToHost, r.st));
    GCHK(hipStreamSynchronize(r.st));
    if (cnt[1] <= cnt[0]) { // first[] / flag[] describe `refined` (the later of the two calls)
        GCHK(hipMemcpyAsync(d.label, d.refined, (size_t)r.N * sizeof(int), hipMemcpyDeviceToDevice, r.st));
    } else if (dev_distinct(r, d.label, 0)) {
        return -1;
    }
    if (dev_renumber(r, d.label))
        return -1;
    GCHK(hipMemsetAsync(d.sum_tot, 0, (size_t)r.N * sizeof(double), r.st));
    hipLaunchKernelGGL(k_scatter_add, dim3(r.nbN), dim3(256), 0, r.st, d.label, d.kdeg, r.N, d.sum_tot);
    return 0;
}
static int dev_finish(LeiRun &r, int *community_out) {
    LeiWork &d = r.d;
    const size_t n = (size_t)r.N;
    if (dev_distinct(r, d.label, 0) || dev_renumber(r, d.label) || lei_w2c_all(r, d.label, d.tmp))
        return -1;
    GCHK(hipMemsetAsync(d.s_in, 0, n * sizeof(double), r.st));
    GCHK(hipMemsetAsync(d.sum_tot, 0, n * sizeof(double), r.st));
    hipLaunchKernelGGL(k_scatter_add, dim3(r.nbN), dim3(256), 0, r.st, d.label, d.tmp, r.N, d.s_in);
    hipLaunchKernelGGL(k_scatter_add, dim3(r.nbN), dim3(256), 0, r.st, d.label, d.kdeg, r.N, d.sum_tot);
    GCHK(hipMemcpyAsync(&r.K, d.counts, sizeof(int), hipMemcpyDeviceToHost, r.st));
    GCHK(hipMemcpyAsync(community_out, d.label, n * sizeof(int), hipMemcpyDeviceToHost, r.st));
    GCHK(hipStreamSynchronize(r.st));
    r.s_in.resize((size_t)r.K);
    r.s_tot.resize((size_t)r.K);
    GCHK(hipMemcpyAsync(r.s_in.data(), d.s_in, (size_t)r.K * sizeof(double), hipMemcpyDeviceToHost, r.st));
    GCHK(hipMemcpyAsync(r.s_tot.data(), d.sum_tot, (size_t)r.K * sizeof(double), hipMemcpyDeviceToHost, r.st));
    GCHK(hipEventRecord(r.g->ev1, r.st));
    GCHK(hipStreamSynchronize(r.st));
    return 0;
}

static int renumber(std::vector<int> &c) { // :317-331
    const int N = (int)c.size();
    std::vector<int> map((size_t)N, -1);
    int next = 0;
    for (int i = 0; i < N; i++) {
        if (map[c[i]] == -1)
            map[c[i]] = next++;
        c[i] = map[c[i]];
    }
    return next;
}
static int host_begin(LeiRun &r) {
    r.k.resize((size_t)r.N);
    GCHK(hipMemcpyAsync(r.k.data(), r.d.kdeg, (size_t)r.N * sizeof(double), hipMemcpyDeviceToHost, r.st));
    GCHK(hipStreamSynchronize(r.st));
    for (int i = 0; i < r.N; i++) // the running total in node order
        r.m += r.k[i];
    r.community.resize((size_t)r.N); // (both partitions are read back from the device when they are needed)
    r.refined.resize((size_t)r.N);
    r.sum_tot = r.k;
    return 0;
}
static int host_after_refinement(LeiRun &r) {
    const size_t n = (size_t)r.N;
    GCHK(hipMemcpyAsync(r.community.data(), r.d.label, n * sizeof(int), hipMemcpyDeviceToHost, r.st));
    GCHK(hipMemcpyAsync(r.refined.data(), r.d.refined, n * sizeof(int), hipMemcpyDeviceToHost, r.st));
    GCHK(hipStreamSynchronize(r.st));
    if (renumber(r.refined) <= renumber(r.community)) // (the one that stays is renumbered anyway; renumbering counts the labels)
        r.community = r.refined;
    std::fill(r.sum_tot.begin(), r.sum_tot.end(), 0.0); // node order
    for (int i = 0; i < r.N; i++)
        r.sum_tot[r.community[i]] += r.k[i];
    GCHK(hipMemcpyAsync(r.d.label, r.community.data(), n * sizeof(int), hipMemcpyHostToDevice, r.st));
    GCHK(hipMemcpyAsync(r.d.sum_tot, r.sum_tot.data(), n * sizeof(double), hipMemcpyHostToDevice, r.st));
    return 0;
}
static int host_finish(LeiRun &r, int *community_out) {
    const size_t n = (size_t)r.N;
    GCHK(hipMemcpyAsync(r.community.data(), r.d.label, n * sizeof(int), hipMemcpyDeviceToHost, r.st));
    GCHK(hipStreamSynchronize(r.st));
    r.K = renumber(r.community);
    // per-node terms on the device, accumulation in node order here
    GCHK(hipMemcpyAsync(r.d.label, r.community.data(), n * sizeof(int), hipMemcpyHostToDevice, r.st));
    if (lei_w2c_all(r, r.d.label, r.d.tmp))
        return -1;
    std::vector<double> w2c(n);
    GCHK(hipMemcpyAsync(w2c.data(), r.d.tmp, n * sizeof(double), hipMemcpyDeviceToHost, r.st));
    GCHK(hipEventRecord(r.g->ev1, r.st));
    GCHK(hipStreamSynchronize(r.st));
    r.s_in.assign((size_t)r.K, 0.0);
    r.s_tot.assign((size_t)r.K, 0.0);
    for (int i = 0; i < r.N; i++) {
        r.s_tot[r.community[i]] += r.k[i];
        r.s_in[r.community[i]] += w2c[i];
    }
    memcpy(community_out, r.community.data(), n * sizeof(int));
    return 0;
}
static const LeiBook lei_book_dev = {dev_begin, dev_after_refinement, dev_finish};
static const LeiBook lei_book_host = {host_begin, host_after_refinement, host_finish};

// ───────────────────────── run_leiden (:336-429) ─────────────────────────
// MN_LEIDEN_BATCHED: batch 0 / 1 = the default schedule, whole-graph synchronous sweeps with a pick-less sweep every
// LEI_PICKLESS (run_phase_sync, period > 0); batch < 0 = the same with period -batch; batch > 1 = rounds of `batch` nodes with
// the safe-winner commit rule (run_phase) — also what finishes a synchronous phase that does not settle.  round_cap: what the
// per-round buffers hold — the largest round of the schedule (run_phase's tail rule), a whole sweep's decisions if period.
struct LeiSchedule {
    int period, batch, round_cap;
};
static LeiSchedule lei_schedule(int mode, int batch, int N) {
    LeiSchedule s = {0, batch, batch};
    if (mode != MN_LEIDEN_BATCHED)
        return s;
    if (batch <= 1) {
        s.period = batch < 0 ? -batch : LEI_PICKLESS;
        const char *e = getenv("MN_LEIDEN_BATCH"); // tuning knob: MN_LEIDEN_BATCH=<round size> selects the round schedule
        if (e && atoi(e) > 1) {
            s.period = 0;
            s.batch = std::max(256, atoi(e));
        }
        if (s.period)
            s.batch = lei_round_default(N); // the rounds a synchronous phase falls back to
    }
    int grow_cap, div_unused;
    lei_grow_setting(&grow_cap, &div_unused);
    s.round_cap = (int)std::min<long long>((long long)s.batch * grow_cap, std::max(s.batch, N));
    if (s.period)
        s.round_cap = std::max(s.round_cap, N);
    return s;
}

// the kernels' arguments that hold for the whole run (a phase sets label / sum_tot / elig_part, a round its range)
static LeiArgs lei_args(const LeiRun &r, double resolution, int max_deg) {
    const LeiWork &d = r.d;
    LeiArgs a;
    memset(&a, 0, sizeof(a));
    a.g = r.dg;
    a.kdeg = d.kdeg;
    a.m = r.m;
    a.resolution = resolution;
    a.use_both = r.use_both;
    a.scratch_c = d.sc, a.scratch_w = d.sw, a.scratch_e = d.se;
    a.max_deg = max_deg;
    a.out = d.out;
    a.max_sweeps = 100000;
    a.dec = d.dec, a.dk = d.dk, a.win = d.win, a.mv = d.mv; // a round's
    a.cmin = d.cmin, a.Jq = d.Jq, a.Lq = d.Lq;              // per community
    a.apply_on_device = r.g->weighted ? 0 : 1;
    a.lds_cap = std::min(LEI_CAP, std::max(64, (max_deg + 15) & ~15));
    a.big_log2h = 8; // a wide node's table: one entry per edge at most (only other communities enter it)
    while ((1 << a.big_log2h) < a.lds_cap)
        a.big_log2h++;
    a.sg_log2h = LEI_SG_LOG2H;
    a.biglist = d.biglist, a.bigoff = d.bigoff;
    return a;
}

static int leiden_impl(mn_graph *g, mn_comm *c, double resolution, int use_both, int mode, int batch, int *community_out,
                       double *modularity_out) {
    GCHK(hipSetDevice(g->device));
    const int N = g->n, nbN = (N + 255) / 256;
    memset(&g->stats, 0, sizeof(g->stats));
    if (modularity_out)
        *modularity_out = 0.0;
    if (N == 0) // :338-339
        return 0;
    const LeiSchedule s = lei_schedule(mode, batch, N);
    const int max_deg = ((use_both ? g->max_deg_both : g->max_deg_out) + 7) & ~3; // int4-aligned scratch stride
    if (lei_prepare(g, mode, s.round_cap, use_both, max_deg))
        return -1;
    hipStream_t st = g->stream;
    LeiWork &d = *g->work;
    LeiRun r = {g, c, d, dev_graph_of(g), st, N, nbN, use_both};
    const LeiBook &book = !g->weighted && mode == MN_LEIDEN_BATCHED ? lei_book_dev : lei_book_host;
    GCHK(hipEventRecord(g->ev0, st));
    hipLaunchKernelGGL(k_wdeg, dim3(nbN), dim3(256), 0, st, r.dg, use_both, d.kdeg); // k[i], m (:344-350)
    if (book.begin(r))
        return -1;
    r.m /= 2.0;
    if (r.m <= 0.0) { // :351-356
        for (int i = 0; i < N; i++)
            community_out[i] = i;
        return 0;
    }
    hipLaunchKernelGGL(k_iota, dim3(nbN), dim3(256), 0, st, d.label, N); // :358-365
    GCHK(hipMemcpyAsync(d.sum_tot, d.kdeg, (size_t)N * sizeof(double), hipMemcpyDeviceToDevice, st));
    LeiArgs a = lei_args(r, resolution, max_deg);
    const auto phase = [&](int64_t *sweeps) {
        return s.period ? run_phase_sync(g, c, a, s.period, sweeps) : run_phase(g, a, mode, s.batch, sweeps);
    };
    for (int iter = 0; iter < 100; iter++) { // :368-417
        a.label = d.label; // local moving (:372)
        a.sum_tot = d.sum_tot;
        a.elig_part = nullptr;
        const long long moves = phase(&g->stats.move_sweeps);
        if (moves < 0)
            return -1;
        g->stats.iterations++;
        g->stats.moves += moves;
        if (moves == 0)
            break;
        // refinement (:383, :238-312): singletons, r_sum_tot = k, moves inside the phase-1 communities only
        hipLaunchKernelGGL(k_iota, dim3(nbN), dim3(256), 0, st, d.refined, N);
        GCHK(hipMemcpyAsync(d.tmp, d.kdeg, (size_t)N * sizeof(double), hipMemcpyDeviceToDevice, st));
        a.label = d.refined;
        a.sum_tot = d.tmp;
        a.elig_part = d.label;
        if (phase(&g->stats.refine_sweeps) < 0 || book.after_refinement(r)) // :385-416
            return -1;
    }
    if (book.finish(r, community_out)) // :420, and compute_modularity's sums (:109-127)
        return -1;
    double Q = 0.0; // :128-139, communities in order (K terms)
    for (int q = 0; q < r.K; q++)
        if (r.s_tot[q] > 0)
            Q += r.s_in[q] / (2.0 * r.m) - resolution * (r.s_tot[q] / (2.0 * r.m)) * (r.s_tot[q] / (2.0 * r.m));
    float ms = 0;
    if (hipEventElapsedTime(&ms, g->ev0, g->ev1) == hipSuccess)
        g->stats.device_ms = ms;
    g->stats.n_communities = r.K;
    if (modularity_out)
        *modularity_out = Q;
    return 0;
}

extern "C" int mn_graph_leiden(mn_graph *g, double resolution, int use_both, int mode, int batch, int *community_out,
                               double *modularity_out) try {
    return leiden_impl(g, nullptr, resolution, use_both, mode, batch, community_out, modularity_out);
} MN_GUARD_END(gset_err, MN_NOTHING, -1)

// run_leiden on the GPUs of a communicator (north_star: the local-move sweep "partitioned across the GPUs ... modularity
// partials").  Every rank holds the whole graph; the parallel schedule's sweeps are divided by node range
// (run_phase_sync) and so are the modularity's per-node terms (lei_w2c_all).  Every rank returns the communities and Q that
// mn_graph_leiden(MN_LEIDEN_BATCHED, batch) returns on one GPU, bit for bit.  batch as there (0: the default schedule).
extern "C" int mn_graph_leiden_shared(mn_graph *g, mn_comm *c, double resolution, int use_both, int batch, int *community_out,
                                      double *modularity_out) try {
    if (c && c->world > 64) {
        gset_err("mn_graph_leiden_shared: more than 64 ranks");
        return -1;
    }
    return leiden_impl(g, c, resolution, use_both, MN_LEIDEN_BATCHED, batch, community_out, modularity_out);
} MN_GUARD_END(gset_err, MN_NOTHING, -1)

extern "C" int mn_graph_leiden_stats(mn_graph *g, mn_leiden_stats *out) try {
    *out = g->stats;
    return 0;
} MN_GUARD_END(gset_err, MN_NOTHING, -1)
