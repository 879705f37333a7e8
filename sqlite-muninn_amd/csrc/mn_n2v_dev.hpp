// mn_n2v_dev.hpp — what a wavefront does in either Node2Vec schedule (k_n2v_seq in mn_n2v.hip, k_n2v_walk_grad in
// mn_n2v_batched.hpp): the reference's xorshift32 stream, the kernels' argument block, the sigmoid LUT lookup and the one
// biased transition step of biased_walk (src/node2vec.c:186-217).
#pragma once
#include <hip/hip_runtime.h>

#define DEVI __device__ __forceinline__
#define N2V_SIG_SIZE 1000
#define N2V_MAX_SIG 6.0f
#define N2V_NEG_TABLE 100000
#define N2V_LDS_DEG 2048 // running totals of one step kept in LDS up to this degree: the sequential schedule's one wavefront
#define N2VB_LDS_DEG 512 // the same for the batched schedule, whose wavefronts share a CU's LDS
#define N2V_LDS_WALK 4096

__host__ __device__ __forceinline__ unsigned xs32(unsigned &s) { // :27-34 (the host draws syn0 from the same stream, :323-325)
    unsigned x = s;
    x ^= x << 13;
    x ^= x >> 17;
    x ^= x << 5;
    s = x;
    return x;
}
DEVI double xs_rand(unsigned &s) { return (double)xs32(s) / (double)0xFFFFFFFFu; } // :36-38

// running-total array of one walk step: LDS when it fits, else global scratch through L2 (sc1)
DEVI double cum_ld(const double *lds, const double *glb, bool in_lds, int i) {
    return in_lds ? lds[i] : __hip_atomic_load(glb + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
DEVI void cum_st(double *lds, double *glb, bool in_lds, int i, double v) {
    if (in_lds)
        lds[i] = v;
    else
        __hip_atomic_store(glb + i, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// the walk: LDS when it fits, else the session's walk scratch through L2 (sc1) — the slots are rewritten every walk
DEVI int walk_ld(const int *lds, const int *glb, bool in_lds, int i) {
    return in_lds ? lds[i] : __hip_atomic_load(glb + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
DEVI void walk_st(int *lds, int *glb, bool in_lds, int i, int v) {
    if (in_lds)
        lds[i] = v;
    else
        __hip_atomic_store(glb + i, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

struct N2vArgs {
    int n;
    const int *off, *adj;
    float *syn0, *syn1neg;
    const int *neg_table;
    const float *sig_table;
    int dim, num_walks, walk_length, window, neg, epochs;
    double p, q, lr;
    unsigned rng;
    double *cum_scratch; // [max_deg] for nodes with more than N2V_LDS_DEG neighbours
    int *walk_scratch;   // [walk_length], used when longer than N2V_LDS_WALK
    unsigned long long *out; // [0] pairs, [1] final rng
};

DEVI float fast_sigmoid(const float *tab, float x) { // :260-271
    if (x >= N2V_MAX_SIG)
        return 1.0f;
    if (x <= -N2V_MAX_SIG)
        return 0.0f;
    int idx = (int)((x + N2V_MAX_SIG) / (2.0f * N2V_MAX_SIG) * N2V_SIG_SIZE);
    if (idx < 0)
        idx = 0;
    if (idx > N2V_SIG_SIZE)
        idx = N2V_SIG_SIZE;
    return tab[idx];
}

// One biased transition of a wavefront standing on the node whose deg > 0 neighbours start at adj[c0], having come from prev:
// returns the next node.  The running totals live in cum_l (LDS) up to LDS_DEG neighbours, in cum_g (global) beyond.  Every lane
// draws the same r from its own copy of the stream.
template <int LDS_DEG>
DEVI int n2v_biased_pick(const N2vArgs &a, int c0, int deg, int prev, double *cum_l, double *cum_g, int lane, unsigned &rng) {
    const bool in_lds = deg <= LDS_DEG;
    const int p0 = a.off[prev], degp = a.off[prev + 1] - p0;
    __builtin_amdgcn_wave_barrier();
    for (int i = lane; i < deg; i += 64) { // transition weights, :186-195
        const int x = a.adj[c0 + i];
        double wt;
        if (x == prev) {
            wt = 1.0 / a.p;
        } else {
            bool nb = false;
            for (int j = 0; j < degp; j++)
                if (a.adj[p0 + j] == x) {
                    nb = true;
                    break;
                }
            wt = nb ? 1.0 : 1.0 / a.q;
        }
        cum_st(cum_l, cum_g, in_lds, i, wt);
    }
    __builtin_amdgcn_s_waitcnt(0);
    __builtin_amdgcn_wave_barrier();
    if (lane == 0) { // Σ in list order, f64 (:196, :213) → running totals
        double t = 0.0;
        for (int i = 0; i < deg; i++) {
            t += cum_ld(cum_l, cum_g, in_lds, i);
            cum_st(cum_l, cum_g, in_lds, i, t);
        }
    }
    __builtin_amdgcn_s_waitcnt(0);
    __builtin_amdgcn_wave_barrier();
    const double total = cum_ld(cum_l, cum_g, in_lds, deg - 1);
    const double r = xs_rand(rng) * total; // :200
    int ci = 0x7fffffff;
    for (int i = lane; i < deg; i += 64)
        if (r <= cum_ld(cum_l, cum_g, in_lds, i)) { // first i with r <= cumulative (:214-217)
            ci = i;
            break;
        }
    for (int m = 32; m >= 1; m >>= 1) {
        int o = __shfl_xor(ci, m);
        ci = o < ci ? o : ci;
    }
    return ci == 0x7fffffff ? a.adj[c0] : a.adj[c0 + ci]; // fallback :202
}
