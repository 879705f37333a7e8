// mn_n2v.hip — Node2Vec biased walks + skip-gram negative sampling (src/node2vec.c:154-394,:486-551)
// on gfx950.
//
// The reference is ONE serial stochastic-gradient stream: a single xorshift32 state feeds the walk
// sampler and the negative sampler alike (:486,:514,:529), every pair updates the embedding rows in
// place, and every f32 dot product is a left-to-right chain over d (:372-375).
//   k_n2v_seq (MN_N2V_SEQUENTIAL)  one wavefront replays that stream exactly: lanes parallelise inside
//        a step (transition weights of the ≤deg neighbours, is_neighbor scans, the dim products, the
//        row updates) while every order-sensitive reduction (Σ weights in f64, the dot chain in f32)
//        is carried out in the reference's order.  Embedding rows are accessed with agent-scope
//        relaxed atomics (L2-served) because the wavefront re-reads rows it has just written.
//        Output bytes are identical to what the reference INSERTs into the output table.
//   k_n2v_normalize                L2 normalisation (:540-551), one wavefront per row, same chain order.
// Host side prepares exactly what the reference prepares serially before training: syn0 from the RNG
// stream (:323-325), the (deg+1)^0.75 negative table (:284-303, f64 pow) and the 1001-entry sigmoid
// LUT (:247-258, expf) — these are inputs of the hot loop, not part of it.
//
// One translation unit (a second one would instantiate rocPRIM's radix sort again), four files:
//   mn_n2v_dev.hpp      what a wavefront does in either schedule: the RNG stream, N2vArgs, the biased transition step
//   mn_n2v_batched.hpp  MN_N2V_BATCHED: its kernels, the session, n2v_samples / n2v_apply
//   mn_n2v_shared.hpp   the batched schedule over several GPUs: the exchange's kernels and buffers, mn_node2vec_train_shared
//   mn_n2v.hip          the two kernels above, the error string, session_init and the other entry points
#include "mn_n2v_shared.hpp"

#include <chrono>
#include <cmath>
#include <cstdarg>

DEVI float ldf(const float *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
DEVI void stf(float *p, float v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__global__ void __launch_bounds__(64) k_n2v_seq(N2vArgs a) {
    extern __shared__ __align__(16) unsigned char smem[];
    const int lane = threadIdx.x;
    double *cum_l = reinterpret_cast<double *>(smem);            // [N2V_LDS_DEG]
    float *prod = reinterpret_cast<float *>(cum_l + N2V_LDS_DEG); // [dim]
    float *vc = prod + a.dim;                                     // [dim]
    float *neu = vc + a.dim;                                      // [dim]
    float *sig = neu + a.dim;                                     // [1001]
    int *walk_l = reinterpret_cast<int *>(sig + N2V_SIG_SIZE + 1); // [walk_length] when it fits, else a.walk_scratch
    int *walk_g = a.walk_scratch;
    const bool walk_in_lds = a.walk_length <= N2V_LDS_WALK;
    for (int i = lane; i <= N2V_SIG_SIZE; i += 64)
        sig[i] = a.sig_table[i];
    __builtin_amdgcn_s_waitcnt(0);
    __builtin_amdgcn_wave_barrier();

    unsigned rng = a.rng;
    const int dim = a.dim;
    const int total_words = a.n * a.num_walks * a.walk_length * a.epochs; // :503 — 32-bit, as the reference
    int word_count = 0;
    unsigned long long pairs = 0;
    for (int epoch = 0; epoch < a.epochs; epoch++)
        for (int w = 0; w < a.num_walks; w++)
            for (int n = 0; n < a.n; n++) {
                float lr = (float)(a.lr * (1.0 - (double)word_count / (double)total_words)); // :510-512
                if (lr < (float)(a.lr * 0.0001))
                    lr = (float)(a.lr * 0.0001);
                // ── biased_walk (:168-226) ──
                int wlen;
                {
                    if (lane == 0)
                        walk_st(walk_l, walk_g, walk_in_lds, 0, n);
                    const int s0 = a.off[n], deg0 = a.off[n + 1] - s0;
                    if (deg0 == 0) {
                        wlen = 1;
                    } else {
                        int idx = (int)(xs_rand(rng) * deg0);
                        if (idx >= deg0)
                            idx = deg0 - 1;
                        int cur = a.adj[s0 + idx], prev = n;
                        if (lane == 0)
                            walk_st(walk_l, walk_g, walk_in_lds, 1, cur);
                        wlen = a.walk_length;
                        for (int step = 2; step < a.walk_length; step++) {
                            const int c0 = a.off[cur], deg = a.off[cur + 1] - c0;
                            if (deg == 0) {
                                wlen = step;
                                break;
                            }
                            const int chosen = n2v_biased_pick<N2V_LDS_DEG>(a, c0, deg, prev, cum_l, a.cum_scratch, lane, rng);
                            if (lane == 0)
                                walk_st(walk_l, walk_g, walk_in_lds, step, chosen);
                            prev = cur;
                            cur = chosen;
                        }
                    }
                }
                __builtin_amdgcn_s_waitcnt(0);
                __builtin_amdgcn_wave_barrier();
                // ── skip-gram over the walk (:517-533) ──
                for (int pos = 0; pos < wlen; pos++) {
                    const int center = walk_ld(walk_l, walk_g, walk_in_lds, pos);
                    int cs = pos - a.window, ce = pos + a.window;
                    if (cs < 0)
                        cs = 0;
                    if (ce >= wlen)
                        ce = wlen - 1;
                    float *rowc = a.syn0 + (size_t)center * dim;
                    for (int c = cs; c <= ce; c++) {
                        if (c == pos)
                            continue;
                        const int context = walk_ld(walk_l, walk_g, walk_in_lds, c);
                        // sgns_train_pair (:345-394)
                        __builtin_amdgcn_wave_barrier();
                        for (int d = lane; d < dim; d += 64) {
                            vc[d] = ldf(rowc + d);
                            neu[d] = 0.0f;
                        }
                        for (int s = 0; s <= a.neg; s++) {
                            int target;
                            float label;
                            if (s == 0) {
                                target = context;
                                label = 1.0f;
                            } else {
                                target = a.neg_table[xs32(rng) % N2V_NEG_TABLE];
                                if (target == center || target == context)
                                    continue; // the draw is consumed first (:361-363)
                                label = 0.0f;
                            }
                            float *rowt = a.syn1neg + (size_t)target * dim;
                            __builtin_amdgcn_s_waitcnt(0);
                            __builtin_amdgcn_wave_barrier();
                            float vt_reg[16]; // dim <= 1024 → at most 16 elements per lane
                            for (int d = lane, r = 0; d < dim; d += 64, r++) {
                                vt_reg[r] = ldf(rowt + d);
                                prod[d] = __fmul_rn(vc[d], vt_reg[r]);
                            }
                            __builtin_amdgcn_s_waitcnt(0);
                            __builtin_amdgcn_wave_barrier();
                            float dot = 0.0f; // left-to-right chain (:372-375), every lane redundantly
                            for (int d = 0; d < dim; d++)
                                dot = __fadd_rn(dot, prod[d]);
                            const float sg = fast_sigmoid(sig, dot);
                            const float err = __fmul_rn(__fsub_rn(label, sg), lr);
                            for (int d = lane, r = 0; d < dim; d += 64, r++) {
                                neu[d] = __fadd_rn(neu[d], __fmul_rn(err, vt_reg[r]));  // :382-384
                                stf(rowt + d, __fadd_rn(vt_reg[r], __fmul_rn(err, vc[d]))); // :386-388
                            }
                        }
                        __builtin_amdgcn_s_waitcnt(0);
                        __builtin_amdgcn_wave_barrier();
                        for (int d = lane; d < dim; d += 64) // :391-393
                            stf(rowc + d, __fadd_rn(vc[d], neu[d]));
                        __builtin_amdgcn_s_waitcnt(0);
                        pairs++;
                    }
                    word_count++;
                }
            }
    if (lane == 0) {
        a.out[0] = pairs;
        a.out[1] = rng;
    }
}

// :540-551 — one wavefront per row; the Σ emb[d]² chain in d order
__global__ void __launch_bounds__(64) k_n2v_normalize(float *syn0, int n, int dim) {
    extern __shared__ float row[];
    const int i = blockIdx.x, lane = threadIdx.x;
    if (i >= n)
        return;
    float *emb = syn0 + (size_t)i * dim;
    for (int d = lane; d < dim; d += 64)
        row[d] = emb[d];
    __builtin_amdgcn_s_waitcnt(0);
    __builtin_amdgcn_wave_barrier();
    float norm = 0.0f;
    for (int d = 0; d < dim; d++)
        norm = __fadd_rn(norm, __fmul_rn(row[d], row[d]));
    norm = sqrtf(norm);
    if (norm > 1e-10f)
        for (int d = lane; d < dim; d += 64)
            emb[d] = __fdiv_rn(row[d], norm);
}

// ───────────────────────── host ─────────────────────────

static thread_local std::string g_nerr;
void nset_err(const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    mn_vformat(g_nerr, fmt, ap);
    va_end(ap);
}
extern "C" const char *mn_node2vec_last_error(void) { return g_nerr.c_str(); }

static int valid_params(const mn_n2v_params *prm) { // src/node2vec.c:443-464
    return prm && prm->dim > 0 && prm->dim <= 1024 && prm->p > 0 && prm->q > 0 && prm->num_walks > 0 && prm->walk_length > 0 &&
           prm->window > 0 && prm->neg_samples > 0 && prm->learning_rate > 0 && prm->epochs > 0;
}

// what every training entry point does first: 1 to go on, else its result (0 for an empty graph, -1 with the error set)
int n2v_enter(const char *who, int n, const mn_n2v_params *prm, mn_n2v_stats *stats, bool others_ok) {
    if (stats)
        memset(stats, 0, sizeof(*stats));
    if (n == 0)
        return 0;
    if (!valid_params(prm) || !others_ok) {
        nset_err("%s: invalid parameters (src/node2vec.c:443-464)", who);
        return -1;
    }
    return 1;
}

// uploads the graph and prepares what the reference prepares serially before its loop (sgns_create, :305-330)
static int session_init(mn_n2v_session *S, int n, const int *off, const int *adj, const mn_n2v_params *prm, int device,
                        bool batched) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) {
        nset_err("node2vec: HIP device %d not available (no CPU fallback)", device);
        return -1;
    }
    NCHK(hipSetDevice(device));
    S->device = device;
    const int dim = prm->dim;
    const size_t nd = (size_t)n * dim;
    unsigned rng = 42; // :486
    std::vector<float> syn0(nd);
    for (size_t i = 0; i < nd; i++) // :323-325
        syn0[i] = ((float)((double)xs32(rng) / (double)0xFFFFFFFFu) - 0.5f) / (float)dim;
    std::vector<int> neg(N2V_NEG_TABLE);
    {
        double total = 0.0; // :284-303
        for (int i = 0; i < n; i++)
            total += pow((double)(off[i + 1] - off[i] + 1), 0.75);
        int idx = 0;
        double cum = 0.0;
        for (int i = 0; i < n && idx < N2V_NEG_TABLE; i++) {
            cum += pow((double)(off[i + 1] - off[i] + 1), 0.75) / total;
            while (idx < N2V_NEG_TABLE && (double)idx / N2V_NEG_TABLE < cum)
                neg[idx++] = i;
        }
        while (idx < N2V_NEG_TABLE)
            neg[idx++] = n - 1;
    }
    std::vector<float> sig(N2V_SIG_SIZE + 1);
    for (int i = 0; i <= N2V_SIG_SIZE; i++) { // :247-258
        float x = (float)i / (float)N2V_SIG_SIZE * 2.0f * N2V_MAX_SIG - N2V_MAX_SIG;
        sig[i] = 1.0f / (1.0f + expf(-x));
    }
    S->max_deg = 0;
    for (int i = 0; i < n; i++)
        S->max_deg = std::max(S->max_deg, off[i + 1] - off[i]);
    const size_t ne = (size_t)off[n];
    DevArena &m = S->mem;
    // (+ 64 rows: the data-parallel mode all-gathers equal row shards of up to 64 ranks in place, ceil(n / world) * world rows)
    if (n2v_alloc(m, S->off, (size_t)n + 1) || n2v_alloc(m, S->adj, ne) || n2v_alloc(m, S->neg, N2V_NEG_TABLE) ||
        n2v_alloc(m, S->sig, N2V_SIG_SIZE + 1) || n2v_alloc(m, S->syn0, nd + (size_t)64 * dim) ||
        n2v_alloc(m, S->syn1, nd + (size_t)64 * dim) || n2v_alloc(m, S->pairs, 2))
        return -1;
    NCHK(hipMemcpy(S->off, off, ((size_t)n + 1) * sizeof(int), hipMemcpyHostToDevice));
    if (ne)
        NCHK(hipMemcpy(S->adj, adj, ne * sizeof(int), hipMemcpyHostToDevice));
    NCHK(hipMemcpy(S->neg, neg.data(), N2V_NEG_TABLE * sizeof(int), hipMemcpyHostToDevice));
    NCHK(hipMemcpy(S->sig, sig.data(), sig.size() * sizeof(float), hipMemcpyHostToDevice));
    NCHK(hipMemcpy(S->syn0, syn0.data(), nd * sizeof(float), hipMemcpyHostToDevice));
    NCHK(hipStreamCreateWithFlags(&S->st, hipStreamNonBlocking));
    NCHK(hipMemsetAsync(S->syn1, 0, nd * sizeof(float), S->st));
    NCHK(hipMemsetAsync(S->pairs, 0, 2 * sizeof(unsigned long long), S->st));
    NCHK(hipEventCreate(&S->e0));
    NCHK(hipEventCreate(&S->e1));
    N2vArgs &a = S->a;
    memset(&a, 0, sizeof(a));
    a.n = n;
    a.off = S->off;
    a.adj = S->adj;
    a.syn0 = S->syn0;
    a.syn1neg = S->syn1;
    a.neg_table = S->neg;
    a.sig_table = S->sig;
    a.dim = dim;
    a.num_walks = prm->num_walks;
    a.walk_length = prm->walk_length;
    a.window = prm->window;
    a.neg = prm->neg_samples;
    a.epochs = prm->epochs;
    a.p = prm->p;
    a.q = prm->q;
    a.lr = prm->learning_rate;
    a.rng = rng;
    a.out = S->pairs;
    if (!batched) {
        if (n2v_alloc(m, S->cum, (size_t)S->max_deg) || n2v_alloc(m, S->walk, (size_t)prm->walk_length))
            return -1;
        a.cum_scratch = S->cum;
        a.walk_scratch = S->walk;
        return 0;
    }
    int B = prm->batch_walks;
    if (B <= 0) // ~75 contributions per row and batch at the default walk/window/neg settings
        B = std::min(16384, std::max(1, n / 64));
    B = std::min(B, n);
    S->B = B;
    S->cap = prm->walk_length * 2 * prm->window * (1 + prm->neg_samples);
    S->ns_max = (size_t)(B + 64) * S->cap; // + padding slots when a batch is split over up to 64 ranks
    if (S->ns_max > 0x7fffffffULL) {
        nset_err("node2vec: batch of %d walks x %d samples exceeds 2^31", B, S->cap);
        return -1;
    }
    S->np_max = (size_t)(B + 64) * prm->walk_length;
    const size_t ns = S->ns_max, np = S->np_max;
    if (n2v_alloc(m, S->s_center, ns) || n2v_alloc(m, S->s_target, ns) || n2v_alloc(m, S->s_err, ns) ||
        n2v_alloc(m, S->p_center, np) || n2v_alloc(m, S->p_neu, np * dim) || n2v_alloc(m, S->keys, ns) || n2v_alloc(m, S->vals, ns) ||
        n2v_alloc(m, S->keys_s, ns) || n2v_alloc(m, S->vals_s, ns) || n2v_alloc(m, S->keys_c, ns) ||
        n2v_alloc(m, S->seg, (size_t)n + 1) || n2v_alloc(m, S->seg_c, (size_t)n + 1) || n2v_alloc(m, S->staged, nd))
        return -1;
    if (S->max_deg > N2VB_LDS_DEG && !(a.p == 1.0 && a.q == 1.0) && n2v_alloc(m, S->cum, (size_t)B * S->max_deg))
        return -1;
    S->bits = 1;
    while ((1u << S->bits) <= (unsigned)n)
        S->bits++;
    if (rocprim::radix_sort_pairs(nullptr, S->tmp_bytes, S->keys, S->keys_s, S->vals, S->vals_s, S->ns_max, 0, S->bits, S->st) !=
        hipSuccess) {
        nset_err("rocprim::radix_sort_pairs (size query) failed");
        return -1;
    }
    return n2v_alloc(m, S->tmp, S->tmp_bytes);
}

extern "C" mn_n2v_session *mn_n2v_begin(int n, const int *off, const int *adj, const mn_n2v_params *prm, int device) try {
    if (n <= 0 || !valid_params(prm)) {
        nset_err("mn_n2v_begin: invalid parameters");
        return nullptr;
    }
    std::unique_ptr<mn_n2v_session> S(new mn_n2v_session());
    if (session_init(S.get(), n, off, adj, prm, device, true) != 0)
        return nullptr;
    (void)hipEventRecord(S->e0, S->st);
    return S.release();
} MN_GUARD_END(nset_err, MN_NOTHING, nullptr)
extern "C" int mn_n2v_batch_walks(mn_n2v_session *S) { return S->B; }
extern "C" int mn_n2v_sample_slots(mn_n2v_session *S) { return S->cap; }
extern "C" int mn_n2v_position_slots(mn_n2v_session *S) { return S->a.walk_length; }
extern "C" int mn_n2v_samples(mn_n2v_session *S, int epoch, int w, int lo, int hi, int *d_center, int *d_target, float *d_err,
                              int *d_pcenter, float *d_pneu) try {
    NCHK(hipSetDevice(S->device));
    if (lo < 0 || hi > S->a.n || hi <= lo || hi - lo > S->B) {
        nset_err("mn_n2v_samples: bad walk range [%d, %d)", lo, hi);
        return -1;
    }
    return n2v_samples(S, epoch, w, lo, hi, d_center, d_target, d_err, d_pcenter, d_pneu);
} MN_GUARD_END(nset_err, MN_NOTHING, -1)
extern "C" int mn_n2v_apply(mn_n2v_session *S, const int *d_center, const int *d_target, const float *d_err, int64_t ns,
                            const int *d_pcenter, const float *d_pneu, int64_t np) try {
    NCHK(hipSetDevice(S->device));
    return n2v_apply(S, d_center, d_target, d_err, ns, d_pcenter, d_pneu, np);
} MN_GUARD_END(nset_err, MN_NOTHING, -1)
extern "C" int mn_n2v_sync(mn_n2v_session *S) try {
    NCHK(hipSetDevice(S->device));
    NCHK(hipDeviceSynchronize());
    return 0;
} MN_GUARD_END(nset_err, MN_NOTHING, -1)
// L2 normalise and leave the embeddings where they are: *d_out = [n][dim] f32 in HBM on the session's device, valid until
// mn_n2v_end (config 4's "-> hnsw index" leg feeds them to mn_hnsw_build_dev without a host round trip)
extern "C" int mn_n2v_finish_dev(mn_n2v_session *S, const float **d_out, mn_n2v_stats *stats) try {
    NCHK(hipSetDevice(S->device));
    const int n = S->a.n, dim = S->a.dim;
    hipLaunchKernelGGL(k_n2v_normalize, dim3(n), dim3(64), (size_t)dim * sizeof(float), S->st, S->syn0, n, dim);
    NCHK(hipEventRecord(S->e1, S->st));
    NCHK(hipStreamSynchronize(S->st));
    unsigned long long o[2];
    NCHK(hipMemcpy(o, S->pairs, sizeof(o), hipMemcpyDeviceToHost));
    *d_out = S->syn0;
    if (stats) {
        float ms = 0;
        (void)hipEventElapsedTime(&ms, S->e0, S->e1);
        stats->pairs = (int64_t)o[0];
        stats->device_ms = ms;
    }
    return n;
} MN_GUARD_END(nset_err, MN_NOTHING, -1)
// the same, and the download (after everything else on the device has come to rest, too)
extern "C" int mn_n2v_finish(mn_n2v_session *S, float *out, mn_n2v_stats *stats) try {
    const float *d_emb = nullptr;
    const int n = mn_n2v_finish_dev(S, &d_emb, stats);
    if (n < 0)
        return -1;
    NCHK(hipDeviceSynchronize());
    NCHK(hipMemcpy(out, d_emb, (size_t)n * S->a.dim * sizeof(float), hipMemcpyDeviceToHost));
    return n;
} MN_GUARD_END(nset_err, MN_NOTHING, -1)

extern "C" void mn_n2v_end(mn_n2v_session *S) {
    if (!S)
        return;
    (void)hipSetDevice(S->device);
    (void)hipDeviceSynchronize();
    delete S;
}

// every batch of every (epoch, w) pass through the session's own sample and position arrays
static int n2v_run_batches(mn_n2v_session *S) {
    const N2vArgs &a = S->a;
    for (int epoch = 0; epoch < a.epochs; epoch++)
        for (int w = 0; w < a.num_walks; w++)
            for (int b0 = 0; b0 < a.n; b0 += S->B) {
                const int b1 = std::min(a.n, b0 + S->B);
                if (n2v_samples(S, epoch, w, b0, b1, S->s_center, S->s_target, S->s_err, S->p_center, S->p_neu) ||
                    n2v_apply(S, S->s_center, S->s_target, S->s_err, (int64_t)(b1 - b0) * S->cap, S->p_center, S->p_neu,
                              (int64_t)(b1 - b0) * a.walk_length))
                    return -1;
            }
    return 0;
}

// node2vec_train's compute followed by its output step (src/node2vec.c:540-583: INSERT every embedding into the output
// hnsw_index) with the embeddings never leaving HBM: trained and normalised on the index's device, then handed to
// mn_hnsw_build_dev with rowids first_rowid + i (the reference's rowid = first-seen index + 1).  host_out (or NULL) also
// receives the embeddings — one bulk copy, for a host that persists them (the extension's "{t}_nodes" shadow table).
// Same embedding bytes as mn_node2vec_train, same graph as mn_hnsw_build on them.  Returns n, or -1.
extern "C" int mn_node2vec_train_into(int n, const int *off, const int *adj, const mn_n2v_params *prm, int mode, mn_index *idx,
                                      int64_t first_rowid, float *host_out, mn_n2v_stats *stats, double *build_seconds) try {
    if (build_seconds)
        *build_seconds = 0.0;
    const int pre = n2v_enter("mn_node2vec_train_into", n, prm, stats, idx != nullptr);
    if (pre <= 0)
        return pre;
    if (mode != MN_N2V_BATCHED) {
        nset_err("mn_node2vec_train_into: MN_N2V_BATCHED only (the serial stream is latency-bound: nothing to gain from HBM residency)");
        return -1;
    }
    N2vSessionPtr S(mn_n2v_begin(n, off, adj, prm, mn_hnsw_device(idx)));
    if (!S)
        return -1;
    const float *d_emb = nullptr;
    if (n2v_run_batches(S.get()) != 0 || mn_n2v_finish_dev(S.get(), &d_emb, stats) < 0)
        return -1;
    std::vector<int64_t> ids((size_t)n);
    for (int i = 0; i < n; i++)
        ids[(size_t)i] = first_rowid + i;
    const auto t0 = std::chrono::steady_clock::now();
    if (mn_hnsw_build_dev(idx, ids.data(), d_emb, n, 0, 0) != 0 || mn_hnsw_sync(idx) != 0) {
        nset_err("mn_node2vec_train_into: %s", mn_last_error());
        return -1;
    }
    if (build_seconds)
        *build_seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    if (host_out && hipMemcpy(host_out, d_emb, (size_t)n * prm->dim * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess) {
        nset_err("mn_node2vec_train_into: download of the embeddings failed");
        return -1;
    }
    return n;
} MN_GUARD_END(nset_err, MN_NOTHING, -1)

extern "C" int mn_node2vec_train(int n, const int *off, const int *adj, const mn_n2v_params *prm, int mode, int device,
                                 float *out, mn_n2v_stats *stats) try {
    const int pre = n2v_enter("mn_node2vec_train", n, prm, stats);
    if (pre <= 0)
        return pre;
    if (mode == MN_N2V_BATCHED) {
        N2vSessionPtr S(mn_n2v_begin(n, off, adj, prm, device));
        if (!S || n2v_run_batches(S.get()) != 0 || mn_n2v_finish(S.get(), out, stats) < 0)
            return -1;
        return n;
    }
    if (mode != MN_N2V_SEQUENTIAL) {
        nset_err("mn_node2vec_train: mode %d not available", mode);
        return -1;
    }
    mn_n2v_session sess;
    mn_n2v_session *S = &sess;
    if (session_init(S, n, off, adj, prm, device, false) != 0)
        return -1;
    const int dim = prm->dim;
    // (a walk longer than N2V_LDS_WALK lives in a.walk_scratch; walk[1] is stored before walk_length is looked at, :178)
    const int walk_lds = prm->walk_length <= N2V_LDS_WALK ? std::max(prm->walk_length, 2) : 0;
    size_t lds = N2V_LDS_DEG * sizeof(double) + 3 * (size_t)dim * sizeof(float) + (N2V_SIG_SIZE + 1) * sizeof(float) +
                 (size_t)walk_lds * sizeof(int) + 64;
    NCHK(hipEventRecord(S->e0, S->st));
    hipLaunchKernelGGL(k_n2v_seq, dim3(1), dim3(64), lds, S->st, S->a);
    NCHK(hipGetLastError());
    return mn_n2v_finish(S, out, stats) < 0 ? -1 : n;
} MN_GUARD_END(nset_err, MN_NOTHING, -1)
