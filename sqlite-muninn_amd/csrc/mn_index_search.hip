// mn_index_search.hip — the search drivers of the mn_index handle (mn_index_int.hpp): the search workspace, the batched, few-queries,
// single and sharded HNSW searches and their overflow checks, brute force, exact search and the exact k-NN graph.  Host code only.
#include "mn_index_int.hpp"

#include <cstdio>

// ───────────────────────── search ─────────────────────────

// allocations of a search launch over nq queries (the only step of it that can fail for lack of memory)
static int reserve_search_ws(mn_index *x, int64_t nq, int ef) {
    hipStream_t st = x->stream;
    if (x->ws_bm0.reserve((size_t)nq * bm0_words(x->n_slots), false, st)) return -1;
    if (x->ws_cand.reserve((size_t)nq * cand_gcap(ef), false, st)) return -1;
    if (x->ws_res.reserve((size_t)nq * res_gcap(ef), false, st)) return -1;
    if (x->ws_counters.reserve(8, false, st)) return -1; // MnSearchArgs::counters
    return 0;
}

int prepare_search_ws(mn_index *x, int64_t nq, int ef, MnSearchArgs &a, bool zero_counters, bool lds_bitmap_ok) {
    hipStream_t st = x->stream;
    a.bm0_words = bm0_words(x->n_slots);
    a.cand_gcap = cand_gcap(ef);
    a.res_gcap = res_gcap(ef);
    if (reserve_search_ws(x, nq, ef))
        return -1;
    // few queries on a small index (the SQL surface: one query per xFilter): k_beam_coop keeps the visited bitmap in LDS
    a.lds_bitmap = lds_bitmap_ok && nq <= 128 &&
                   (long long)mn_search_lds_bytes(x->ld, true) + 1024 + a.bm0_words * (long long)sizeof(unsigned) <= 64 * 1024 &&
                   !(getenv("MN_COOP") && atoi(getenv("MN_COOP")) == 0) && !(getenv("MN_LDS_BITMAP") && atoi(getenv("MN_LDS_BITMAP")) == 0);
    if (!a.lds_bitmap)
        HIPCHK(hipMemsetAsync(x->ws_bm0.p, 0, (size_t)nq * a.bm0_words * sizeof(unsigned), st));
    if (zero_counters)
        HIPCHK(hipMemsetAsync(x->ws_counters.p, 0, 8 * sizeof(unsigned long long), st));
    a.bitmap0 = x->ws_bm0.p;
    a.cand_ovf = x->ws_cand.p;
    a.res_ovf = x->ws_res.p;
    a.counters = x->ws_counters.p;
    a.bitmap_up = nullptr;
    a.bmu_words = 0;
    a.no_spec_rows = mn_no_spec_rows(x->n_slots, x->ld);
#ifdef MN_SSE_TILE_PATH
    const char *e = getenv("MN_SSE_TILE"); // tuning knob of the opt-in tiled SSE path
    a.use_tile = e ? atoi(e) : 1;
#else
    a.use_tile = 0;
#endif
    return 0;
}

void last_from_counters(mn_index *x, const unsigned long long *c, bool timed) {
    float ms = 0;
    if (!timed)
        x->last.last_kernel_ms = 0.0f;
    else if (hipEventElapsedTime(&ms, x->ev0, x->ev1) == hipSuccess)
        x->last.last_kernel_ms = ms;
    x->last.last_n_dist = (int64_t)c[0];
    x->last.last_n_expanded = (int64_t)c[1];
    x->last.last_n_overflow = (int64_t)c[2];
    x->last.last_n_exact_rows = (int64_t)(c[0] - c[3]); // ([3]: distances the shadow's bound decided alone)
    x->last.last_n_rows_lanes8 = (int64_t)c[4];
    x->last.last_n_rows_lanes16 = (int64_t)c[5];
    x->last.last_n_rows_lanes4 = x->last.last_n_exact_rows - (int64_t)(c[4] + c[5]);
}

int fetch_counters(mn_index *x) {
    unsigned long long c[8];
    if (!x->ws_counters.p) // nothing launched yet
        return 0;
    HIPCHK(hipMemcpyAsync(c, x->ws_counters.p, sizeof(c), hipMemcpyDeviceToHost, x->stream));
    HIPCHK(hipStreamSynchronize(x->stream));
    last_from_counters(x, c, true);
    return 0;
}

// q_counters: see MnSearchArgs (the few-queries path: the stream then carries the search kernel and nothing else — no counter
// memset, no event records, no copy back)
static int search_batch_dev_impl(mn_index *x, const float *d_queries, int64_t nq, int k, int ef, int64_t *d_ids, float *d_dists,
                                 int *d_counts, unsigned long long *q_counters) {
    if (use_device(x))
        return -1;
    if (nq <= 0)
        return 0;
    if (k <= 0) {
        set_err("mn_hnsw_search: k must be > 0");
        return -1;
    }
    if (ef < k) // src/hnsw_algo.c:673
        ef = k;
    hipStream_t st = x->stream;
    if (x->entry_id == -1 || x->node_count == 0) { // :671
        HIPCHK(hipMemsetAsync(d_counts, 0, (size_t)nq * sizeof(int), st));
        HIPCHK(hipMemsetAsync(d_ids, 0xFF, (size_t)nq * k * sizeof(int64_t), st));
        HIPCHK(hipMemsetAsync(d_dists, 0, (size_t)nq * k * sizeof(float), st));
        return 0;
    }
    if (push_links(x) || sync_meta(x))
        return -1;
    // per-query workspace (visited bitmap + heap spill) is bounded to ~8 GiB: larger batches run as chunks
    const size_t per_q = search_ws_bytes_per_query(x->n_slots, ef);
    const int64_t chunk = std::max<int64_t>(1, std::min<int64_t>(nq, (int64_t)((8ull << 30) / per_q)));
    const int entry_slot = ht_find(x, x->entry_id);
    MnDevIndex v = dev_view(x);
    // every allocation happens here, for the largest chunk: nothing between the two event records can fail half-way
    if (reserve_search_ws(x, chunk, ef))
        return -1;
    if (!q_counters) {
        HIPCHK(hipEventRecord(x->ev0, st));
        x->last_on_host = false;
    }
    for (int64_t q0 = 0; q0 < nq; q0 += chunk) {
        const int64_t m = std::min<int64_t>(chunk, nq - q0);
        MnSearchArgs a;
        memset(&a, 0, sizeof(a));
        if (prepare_search_ws(x, m, ef, a, q0 == 0 && !q_counters, true)) { // (sized above: memsets only)
            if (!q_counters)
                (void)hipEventRecord(x->ev1, st);
            return -1;
        }
        a.q_counters = q_counters ? q_counters + (size_t)q0 * MN_QC : nullptr;
        a.queries = d_queries + (size_t)q0 * x->dim;
        a.nq = m;
        a.k = k;
        a.ef = ef;
        a.entry_slot = entry_slot;
        a.max_level = x->max_level;
        a.out_ids = (long long *)d_ids + (size_t)q0 * k;
        a.out_dists = d_dists + (size_t)q0 * k;
        a.out_counts = d_counts + q0;
        mn_launch_search(v, a, false, st);
    }
    if (!q_counters)
        HIPCHK(hipEventRecord(x->ev1, st));
    HIPCHK(hipGetLastError());
    return 0;
}

extern "C" int mn_hnsw_search_batch_dev(mn_index *x, const float *d_queries, int64_t nq, int k, int ef, int64_t *d_ids,
                                        float *d_dists, int *d_counts) try {
    return search_batch_dev_impl(x, d_queries, nq, k, ef, d_ids, d_dists, d_counts, nullptr);
} MN_GUARD_END(set_err, MN_NOTHING, -1)

// A sharded search all-gathers every shard's overflow count next to its top-k (mn_hnsw_search_sharded_dev): every rank sees
// the same counts, so every rank fails alike — and names the shard — the first time its host looks (any synchronising call).
static int check_sharded_overflow(mn_index *x) {
    if (!x->sh_ovf_pending)
        return 0;
    const int world = x->sh_ovf_pending;
    x->sh_ovf_pending = 0;
    std::vector<unsigned long long> h((size_t)world);
    HIPCHK(hipMemcpyAsync(h.data(), x->sh_ovf.p, (size_t)world * sizeof(unsigned long long), hipMemcpyDeviceToHost, x->stream));
    HIPCHK(hipStreamSynchronize(x->stream));
    for (int r = 0; r < world; r++)
        if (h[(size_t)r]) {
            set_err("mn_hnsw_search_sharded: shard %d: %llu queries exceeded heap workspace (its top-k lists are truncated)", r,
                    h[(size_t)r]);
            return -1;
        }
    return 0;
}

// for mn_shards.hip (one process, several GPUs): synchronises the index's stream and reports an overflow of its last search
int mn_index_search_overflow(mn_index *x, long long *n_overflow) {
    *n_overflow = 0;
    if (x->entry_id == -1 || x->node_count == 0)
        return 0;
    if (fetch_counters(x))
        return -1;
    *n_overflow = (long long)x->last.last_n_overflow;
    return 0;
}

extern "C" int mn_hnsw_sync(mn_index *x) try {
    if (use_device(x))
        return -1;
    HIPCHK(hipStreamSynchronize(x->stream));
    return check_sharded_overflow(x);
} MN_GUARD_END(set_err, MN_NOTHING, -1)

// A handful of queries from host memory: the kernel reads them from, and writes ids / distances / counts to, one pinned host
// block; the counters follow in the same block; ONE synchronisation.
static int search_small(mn_index *x, const float *queries, int64_t nq, int k, int ef, int64_t *out_ids, float *out_dists,
                        int *out_counts) {
    hipStream_t st = x->stream;
    const size_t qb = (size_t)nq * x->dim * sizeof(float), ib = (size_t)nq * k * sizeof(int64_t), db = (size_t)nq * k * sizeof(float);
    const size_t cb = ((size_t)nq * sizeof(int) + 7) & ~(size_t)7;
    const size_t o_ids = (qb + 15) & ~(size_t)15, o_d = o_ids + ib, o_c = (o_d + db + 7) & ~(size_t)7, o_cnt = o_c + cb;
    const size_t need = o_cnt + (size_t)nq * MN_QC * sizeof(unsigned long long);
    if (push_links(x) || sync_meta(x)) // (before the block is written: a pending single-slot upload stages through it too)
        return -1;
    if (!pin_reserve(x, need)) {
        set_err("mn_hnsw_search: cannot allocate %zu bytes of pinned host memory", need);
        return -1;
    }
    HIPCHK(hipStreamSynchronize(st));
    memcpy(x->pin, queries, qb);
    unsigned long long *qc = reinterpret_cast<unsigned long long *>(x->pin + o_cnt);
    if (search_batch_dev_impl(x, (const float *)x->pin, nq, k, ef, (int64_t *)(x->pin + o_ids), (float *)(x->pin + o_d),
                              (int *)(x->pin + o_c), qc))
        return -1;
    const bool launched = x->entry_id != -1 && x->node_count > 0;
    HIPCHK(hipStreamSynchronize(st)); // the one wait of a lone query: the kernel has answered into the block, counters included
    memcpy(out_ids, x->pin + o_ids, ib);
    memcpy(out_dists, x->pin + o_d, db);
    memcpy(out_counts, x->pin + o_c, (size_t)nq * sizeof(int));
    if (launched) {
        unsigned long long tot[MN_QC] = {0, 0, 0, 0, 0, 0};
        for (int64_t q = 0; q < nq; q++)
            for (int i = 0; i < MN_QC; i++)
                tot[i] += qc[q * MN_QC + i];
        last_from_counters(x, tot, false); // (not timed: no event records on this path)
        x->last_on_host = true;
        if (x->last.last_n_overflow) {
            set_err("mn_hnsw_search: %lld queries exceeded heap workspace", (long long)x->last.last_n_overflow);
            return -1;
        }
    }
    return 0;
}

// The host-memory entry points: room for the answers of nq queries, k each, in ws_outi / ws_outd / ws_outc and — queries not null —
// the queries uploaded into ws_q; then the device face; then ids, distances and counts back to the host and the wait for them.
template <typename F>
static int with_staged_io(mn_index *x, const float *queries, size_t nq, int k, int64_t *out_ids, float *out_dists, int *out_counts,
                          F &&dev_face) {
    hipStream_t st = x->stream;
    if (queries && x->ws_q.reserve(nq * x->dim, false, st)) return -1;
    if (x->ws_outi.reserve(nq * k, false, st)) return -1;
    if (x->ws_outd.reserve(nq * k, false, st)) return -1;
    if (x->ws_outc.reserve(nq, false, st)) return -1;
    if (queries)
        HIPCHK(hipMemcpyAsync(x->ws_q.p, queries, nq * x->dim * sizeof(float), hipMemcpyHostToDevice, st));
    if (dev_face())
        return -1;
    HIPCHK(hipMemcpyAsync(out_ids, x->ws_outi.p, nq * k * sizeof(int64_t), hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(out_dists, x->ws_outd.p, nq * k * sizeof(float), hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(out_counts, x->ws_outc.p, nq * sizeof(int), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return 0;
}

extern "C" int mn_hnsw_search_batch(mn_index *x, const float *queries, int64_t nq, int k, int ef, int64_t *out_ids,
                                    float *out_dists, int *out_counts) try {
    if (use_device(x))
        return -1;
    if (nq <= 0)
        return 0;
    if (k > 0 && (size_t)nq * ((size_t)x->dim * 4 + (size_t)k * 12 + 4) <= ((size_t)1 << 20))
        return search_small(x, queries, nq, k, ef, out_ids, out_dists, out_counts);
    if (with_staged_io(x, queries, (size_t)nq, k, out_ids, out_dists, out_counts, [&] {
            return mn_hnsw_search_batch_dev(x, x->ws_q.p, nq, k, ef, (int64_t *)x->ws_outi.p, x->ws_outd.p, x->ws_outc.p);
        }))
        return -1;
    if (x->entry_id != -1 && x->node_count > 0) {
        if (fetch_counters(x))
            return -1;
        if (x->last.last_n_overflow) {
            set_err("mn_hnsw_search: %lld queries exceeded heap workspace", (long long)x->last.last_n_overflow);
            return -1;
        }
    }
    return 0;
} MN_GUARD_END(set_err, MN_NOTHING, -1)

extern "C" int mn_hnsw_search(mn_index *x, const float *query, int k, int ef, mn_search_result *results) try {
    if (k <= 0)
        return 0;
    std::vector<int64_t> ids((size_t)k);
    std::vector<float> ds((size_t)k);
    int cnt = 0;
    if (mn_hnsw_search_batch(x, query, 1, k, ef, ids.data(), ds.data(), &cnt))
        return 0; // src/hnsw_algo.h:70: count, 0 on failure
    for (int i = 0; i < cnt; i++) {
        results[i].id = ids[i];
        results[i].distance = ds[i];
    }
    return cnt;
} MN_GUARD_END(set_err, MN_NOTHING, 0)

extern "C" int mn_hnsw_search_sharded_dev(mn_index *x, mn_comm *c, const float *d_queries, int64_t nq, int k, int ef,
                                          int64_t *d_ids, float *d_dists, int *d_counts) try {
    if (use_device(x))
        return -1;
    if (nq <= 0)
        return 0;
    const int world = c ? c->world : 1, rank = c ? c->rank : 0;
    if (world > 64) {
        set_err("mn_hnsw_search_sharded: more than 64 shards");
        return -1;
    }
    hipStream_t st = x->stream;
    const size_t per = (size_t)nq * k;
    if (x->sh_gids.reserve(per * world, false, st) || x->sh_gd.reserve(per * world, false, st) ||
        x->sh_gcnt.reserve((size_t)nq * world, false, st))
        return -1;
    // this shard's top-k straight into its slot of the gather buffers, then the one exchange step, then the merge
    long long *my_ids = x->sh_gids.p + per * rank;
    float *my_d = x->sh_gd.p + per * rank;
    int *my_c = x->sh_gcnt.p + (size_t)nq * rank;
    if (mn_hnsw_search_batch_dev(x, d_queries, nq, k, ef, (int64_t *)my_ids, my_d, my_c))
        return -1;
    // this shard's heap-workspace overflow count travels with its lists: a truncated list must not be merged silently
    if (x->sh_ovf.reserve((size_t)world, false, st))
        return -1;
    if (x->entry_id == -1 || x->node_count == 0 || !x->ws_counters.p)
        HIPCHK(hipMemsetAsync(x->sh_ovf.p + rank, 0, sizeof(unsigned long long), st));
    else
        HIPCHK(hipMemcpyAsync(x->sh_ovf.p + rank, x->ws_counters.p + 2, sizeof(unsigned long long), hipMemcpyDeviceToDevice, st));
    if (const char *fi = getenv("MN_FAULT_INJECT")) { // test hook: "search_overflow:<rank>" = this shard reports 3 truncated lists
        int fr = -1;
        const unsigned long long three = 3;
        if (sscanf(fi, "search_overflow:%d", &fr) == 1 && fr == rank) {
            HIPCHK(hipMemcpyAsync(x->sh_ovf.p + rank, &three, sizeof(three), hipMemcpyHostToDevice, st));
            HIPCHK(hipStreamSynchronize(st));
        }
    }
    x->sh_ovf_pending = world;
    if (world > 1 || (c && c->nccl)) {
        if (mn_comm_allgather_dev(c, my_ids, x->sh_gids.p, per * sizeof(long long), st) ||
            mn_comm_allgather_dev(c, my_d, x->sh_gd.p, per * sizeof(float), st) ||
            mn_comm_allgather_dev(c, x->sh_ovf.p + rank, x->sh_ovf.p, sizeof(unsigned long long), st) ||
            mn_comm_allgather_dev(c, my_c, x->sh_gcnt.p, (size_t)nq * sizeof(int), st)) {
            set_err("mn_hnsw_search_sharded: %s", mn_comm_last_error_str());
            return -1;
        }
    }
    mn_launch_merge_topk(x->sh_gids.p, x->sh_gd.p, x->sh_gcnt.p, world, nq, k, (long long *)d_ids, d_dists, d_counts, st);
    HIPCHK(hipGetLastError());
    return 0;
} MN_GUARD_END(set_err, MN_NOTHING, -1)

extern "C" int mn_hnsw_search_sharded(mn_index *x, mn_comm *c, const float *queries, int64_t nq, int k, int ef, int64_t *out_ids,
                                      float *out_dists, int *out_counts) try {
    if (use_device(x))
        return -1;
    if (nq <= 0)
        return 0;
    if (with_staged_io(x, queries, (size_t)nq, k, out_ids, out_dists, out_counts, [&] {
            return mn_hnsw_search_sharded_dev(x, c, x->ws_q.p, nq, k, ef, (int64_t *)x->ws_outi.p, x->ws_outd.p, x->ws_outc.p);
        }))
        return -1;
    return check_sharded_overflow(x);
} MN_GUARD_END(set_err, MN_NOTHING, -1)

extern "C" int mn_hnsw_bruteforce_topk(mn_index *x, const float *d_queries, int64_t nq, int k, int64_t *out_ids) try {
    if (use_device(x))
        return -1;
    if (push_links(x) || sync_meta(x))
        return -1;
    hipStream_t st = x->stream;
    if (x->ws_outi.reserve((size_t)nq * k, false, st)) return -1;
    const char *force = getenv("MN_BRUTE"); // "valu" = the index's own inner loop (any k <= 128); default: MFMA when k <= 16
    MnDevIndex v = dev_view(x);
    if (k <= 16 && nq > 0 && x->n_slots > 0 && !(force && !strcmp(force, "valu"))) {
        int nc = 0, rpc = 0;
        const size_t bytes = mn_brute_mfma_scratch_bytes(v, nq, k, &nc, &rpc);
        IndexBuf<unsigned char> scratch;
        if (scratch.reserve(bytes, false, st))
            return -1;
        HIPCHK(hipEventRecord(x->ev0, st));
        const int rc = mn_launch_bruteforce_mfma(v, d_queries, nq, k, x->ws_outi.p, scratch.p, st);
        HIPCHK(hipEventRecord(x->ev1, st));
        hipError_t e = hipStreamSynchronize(st);
        if (rc != 0 || e != hipSuccess) {
            set_err("mn_hnsw_bruteforce_topk: MFMA kernel failed (%s)", hipGetErrorString(e));
            return -1;
        }
        float ms = 0;
        if (hipEventElapsedTime(&ms, x->ev0, x->ev1) == hipSuccess)
            x->last.last_kernel_ms = ms;
    } else {
        mn_launch_bruteforce(v, d_queries, nq, k, x->ws_outi.p, nullptr, st);
        HIPCHK(hipGetLastError());
    }
    HIPCHK(hipMemcpyAsync(out_ids, x->ws_outi.p, (size_t)nq * k * sizeof(int64_t), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return 0;
} MN_GUARD_END(set_err, MN_NOTHING, -1)

// ───────────────────────── exact search (mn_exact.hip) ─────────────────────────

// what a call reads from the environment, once: kp = k + MN_EXACT_SLACK list entries per query (default 16; 0: most certificates
// fail), at most 64, and whether the candidate pass runs at all (k <= 32 and not MN_EXACT=valu)
struct ExactPlan {
    int kp;
    bool mfma;
};
static ExactPlan exact_plan(int k) {
    const char *force = getenv("MN_EXACT");         // "valu": the index's inner loop over every row for every query
    const char *slack_e = getenv("MN_EXACT_SLACK"); // list entries beyond k
    int slack = slack_e ? atoi(slack_e) : 16;
    if (slack < 0)
        slack = 0;
    return {std::min(k + slack, 64), k <= 32 && !(force && !strcmp(force, "valu"))};
}
static size_t up256(size_t b) { return (b + 255) & ~(size_t)255; }

// the outputs of one batch and the device scratch its steps share
struct ExactBatch {
    const float *d_queries; // the search's queries; null for the self-join
    const MnExactSelf *self; // the self-join's slots, radius and row constants; null for the search
    long long nq;
    const unsigned *d_allow;
    void *scratch;             // mn_exact_mfma_scratch_bytes
    int *d_marked;             // [nq]
    unsigned long long *d_ctr; // [4]
    long long *o_ids;
    float *o_d;
    int *o_c;
};
// One batch of queries: counters zeroed, the candidate pass with its certificate, then the walk over the queries it marked — or,
// where the pass is off or the device refuses the LDS its lists need, over all of them; plan->mfma is then cleared and tot reset, for
// the whole call takes the walk.  The pass's counters are added to tot [3], the device time of the batch to *ms_sum.
static int exact_batch(mn_index *x, const char *who, const MnDevIndex &v, const ExactBatch &b, int k, ExactPlan *plan,
                       unsigned long long *tot, float *ms_sum) {
    hipStream_t st = x->stream;
    auto fail = [&]() {
        set_err("%s: launch failed (%s)", who, hipGetErrorString(hipGetLastError()));
        (void)hipStreamSynchronize(st);
        return -1;
    };
    HIPCHK(hipMemsetAsync(b.d_ctr, 0, 4 * sizeof(unsigned long long), st));
    HIPCHK(hipEventRecord(x->ev0, st));
    if (plan->mfma) {
        if (b.self && b.self->s0 == 0) // the rows' constants: once per call
            mn_launch_knn_prep_rows(v, b.self->d_xc, st);
        const int rc = mn_launch_exact_mfma(v, b.d_queries, b.nq, k, plan->kp, b.d_allow, b.scratch, b.o_ids, b.o_d, b.o_c, b.d_ctr,
                                            b.d_marked, b.self, st);
        if (rc < 0)
            return fail();
        if (rc == 1) { // the LDS grant is refused (before anything of the pass was launched)
            plan->mfma = false;
            tot[0] = tot[1] = tot[2] = 0;
        }
    }
    if (plan->mfma) {
        unsigned long long ctr[3] = {0, 0, 0};
        HIPCHK(hipMemcpyAsync(ctr, b.d_ctr, sizeof(ctr), hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        // the marked queries alone, in one launch
        if (mn_launch_exact_valu(v, b.d_queries, b.d_marked, (long long)ctr[0], k, b.d_allow, b.o_ids, b.o_d, b.o_c, b.self, st))
            return fail();
        for (int i = 0; i < 3; i++)
            tot[i] += ctr[i];
    } else if (mn_launch_exact_valu(v, b.d_queries, nullptr, b.nq, k, b.d_allow, b.o_ids, b.o_d, b.o_c, b.self, st)) {
        return fail();
    }
    HIPCHK(hipEventRecord(x->ev1, st));
    HIPCHK(hipStreamSynchronize(st));
    float ms = 0;
    if (hipEventElapsedTime(&ms, x->ev0, x->ev1) == hipSuccess)
        *ms_sum += ms;
    return 0;
}

static int exact_search_dev(mn_index *x, const float *d_queries, int64_t nq, int k, const int64_t *allow_ids, int64_t n_allow,
                            int64_t *d_ids, float *d_dists, int *d_counts) {
    if (k < 1 || k > 128 || nq < 0 || n_allow < 0) {
        set_err("mn_hnsw_search_exact: k must be 1..128 (got %d), nq and n_allow >= 0", k);
        return -1;
    }
    if (push_links(x) || sync_meta(x))
        return -1;
    x->last_exact = {nq, 0, 0, 0, 0, 0.0f};
    if (nq == 0)
        return 0;
    hipStream_t st = x->stream;
    if (x->n_slots == 0) {
        mn_launch_exact_fill(nq, k, (long long *)d_ids, d_dists, d_counts, st);
        HIPCHK(hipGetLastError());
        HIPCHK(hipStreamSynchronize(st));
        return 0;
    }
    ExactPlan plan = exact_plan(k);
    MnDevIndex v = dev_view(x);
    // the allow-list as one bit per slot
    const size_t words = allow_ids ? (size_t)bm0_words(x->n_slots) : 0;
    std::vector<unsigned> bits(words, 0u);
    for (int64_t i = 0; allow_ids && i < n_allow; i++) {
        const int s = ht_find(x, allow_ids[i]);
        if (s >= 0 && !x->deleted[s])
            bits[(size_t)s >> 5] |= 1u << (s & 31);
    }
    // one device allocation per call: the pass's scratch | allow bits | marked queries | counters
    const size_t b_mfma = plan.mfma ? mn_exact_mfma_scratch_bytes(v, nq, plan.kp) : 0;
    const size_t b_bits = up256(words * 4), b_marked = up256((size_t)nq * 4);
    IndexBuf<unsigned char> sc;
    if (sc.reserve(b_mfma + b_bits + b_marked + 256, false, st))
        return -1;
    unsigned *d_allow = reinterpret_cast<unsigned *>(sc.p + b_mfma);
    const ExactBatch b = {d_queries, nullptr, nq, allow_ids ? d_allow : nullptr, sc.p, reinterpret_cast<int *>(sc.p + b_mfma + b_bits),
                          reinterpret_cast<unsigned long long *>(sc.p + b_mfma + b_bits + b_marked), (long long *)d_ids, d_dists, d_counts};
    if (words)
        HIPCHK(hipMemcpyAsync(d_allow, bits.data(), words * 4, hipMemcpyHostToDevice, st));
    unsigned long long tot[3] = {0, 0, 0};
    float ms = 0.0f;
    if (exact_batch(x, "mn_hnsw_search_exact", v, b, k, &plan, tot, &ms))
        return -1;
    x->last_exact = {nq, plan.mfma ? nq : 0, (int64_t)tot[0], (int64_t)tot[1], (int64_t)tot[2], ms};
    return 0;
}

extern "C" int mn_hnsw_search_exact_batch_dev(mn_index *x, const float *d_queries, int64_t nq, int k, const int64_t *allow_ids,
                                              int64_t n_allow, int64_t *d_ids, float *d_dists, int *d_counts) try {
    if (use_device(x))
        return -1;
    return exact_search_dev(x, d_queries, nq, k, allow_ids, n_allow, d_ids, d_dists, d_counts);
} MN_GUARD_END(set_err, MN_NOTHING, -1)

extern "C" int mn_hnsw_search_exact_batch(mn_index *x, const float *queries, int64_t nq, int k, const int64_t *allow_ids,
                                          int64_t n_allow, int64_t *out_ids, float *out_dists, int *out_counts) try {
    if (use_device(x))
        return -1;
    if (nq <= 0 || k < 1 || k > 128)
        return exact_search_dev(x, nullptr, nq, k, allow_ids, n_allow, nullptr, nullptr, nullptr);
    return with_staged_io(x, queries, (size_t)nq, k, out_ids, out_dists, out_counts, [&] {
        return exact_search_dev(x, x->ws_q.p, nq, k, allow_ids, n_allow, (int64_t *)x->ws_outi.p, x->ws_outd.p, x->ws_outc.p);
    });
} MN_GUARD_END(set_err, MN_NOTHING, -1)

// ───────────────────────── exact k-NN graph of the index's own rows ─────────────────────────

// Outputs in device memory, indexed by slot.  The slots go through in batches of B queries; per batch the rules of
// exact_search_dev (exact_batch): candidate pass + certificate, the marked queries gathered into one walk; k > 32, MN_EXACT=valu
// and a refused LDS grant walk every row.
static int knn_graph_dev(mn_index *x, int k, float r, int64_t *d_ids, float *d_dists, int *d_counts) {
    if (k < 1 || k > 128) {
        set_err("mn_hnsw_knn_graph: k must be 1..128 (got %d)", k);
        return -1;
    }
    if (r != r) {
        set_err("mn_hnsw_knn_graph: max_distance is NaN");
        return -1;
    }
    if (push_links(x) || sync_meta(x))
        return -1;
    x->last_exact = {0, 0, 0, 0, 0, 0.0f};
    const int n = x->n_slots;
    if (n == 0)
        return 0;
    int64_t n_live = 0;
    for (int s = 0; s < n; s++)
        n_live += x->deleted[s] ? 0 : 1;
    hipStream_t st = x->stream;
    ExactPlan plan = exact_plan(k);
    const char *batch_e = getenv("MN_KNN_BATCH"); // query slots per batch, rounded up to a multiple of 128
    long long B = batch_e ? atoll(batch_e) : 16384;
    if (B < 1)
        B = 16384;
    B = std::min<long long>((B + 127) / 128 * 128, ((long long)n + 127) / 128 * 128);
    MnDevIndex v = dev_view(x);
    // one device allocation per call: a batch's scratch (the last, shorter batch cuts its row chunks differently) | the rows'
    // constants | marked queries | counters
    const long long rem = n % B;
    const size_t b_batch = plan.mfma ? std::max(mn_exact_mfma_scratch_bytes(v, std::min<long long>(B, n), plan.kp, true),
                                                rem ? mn_exact_mfma_scratch_bytes(v, rem, plan.kp, true) : (size_t)0)
                                     : 0;
    const size_t b_xc = plan.mfma ? up256((size_t)n * 8) : 0, b_marked = up256((size_t)B * 4);
    IndexBuf<unsigned char> sc;
    if (sc.reserve(b_batch + b_xc + b_marked + 256, false, st))
        return -1;
    MnExactSelf self = {0, r, sc.p + b_batch};
    ExactBatch b = {nullptr, &self, 0, nullptr, sc.p, reinterpret_cast<int *>(sc.p + b_batch + b_xc),
                    reinterpret_cast<unsigned long long *>(sc.p + b_batch + b_xc + b_marked), nullptr, nullptr, nullptr};
    unsigned long long tot[3] = {0, 0, 0};
    float ms_sum = 0.0f;
    for (long long s0 = 0; s0 < n; s0 += B) {
        self.s0 = (int)s0;
        b.nq = std::min<long long>(B, n - s0);
        b.o_ids = (long long *)d_ids + (size_t)s0 * k;
        b.o_d = d_dists + (size_t)s0 * k;
        b.o_c = d_counts + s0;
        if (exact_batch(x, "mn_hnsw_knn_graph", v, b, k, &plan, tot, &ms_sum))
            return -1;
    }
    x->last_exact = {n_live, plan.mfma ? n_live : 0, (int64_t)tot[0], (int64_t)tot[1], (int64_t)tot[2], ms_sum};
    return 0;
}

extern "C" int mn_hnsw_knn_graph_dev(mn_index *x, int k, float max_distance, int64_t *d_ids, float *d_dists, int *d_counts) try {
    if (use_device(x))
        return -1;
    return knn_graph_dev(x, k, max_distance, d_ids, d_dists, d_counts);
} MN_GUARD_END(set_err, MN_NOTHING, -1)

extern "C" int mn_hnsw_knn_graph(mn_index *x, int k, float max_distance, int64_t *out_ids, float *out_dists, int *out_counts) try {
    if (use_device(x))
        return -1;
    const size_t n = (size_t)x->n_slots;
    if (n == 0 || k < 1 || k > 128 || max_distance != max_distance)
        return knn_graph_dev(x, k, max_distance, nullptr, nullptr, nullptr);
    return with_staged_io(x, nullptr, n, k, out_ids, out_dists, out_counts, [&] {
        return knn_graph_dev(x, k, max_distance, (int64_t *)x->ws_outi.p, x->ws_outd.p, x->ws_outc.p);
    });
} MN_GUARD_END(set_err, MN_NOTHING, -1)

extern "C" int mn_hnsw_last_exact(mn_index *x, mn_exact_stats *out) try {
    *out = x->last_exact;
    return 0;
} MN_GUARD_END(set_err, MN_NOTHING, -1)
