// mn_index_insert.hip — the insert and build drivers of the mn_index handle (mn_index_int.hpp): the search and link halves of a
// batch, the batched, sequential and speculative inserts, the logged insert, the bulk builds, the staged batch API and the
// jointly built graph of several GPUs.  Host code only.
#include "mn_index_int.hpp"

#include <cstdio>

// ───────────────────────── insert ─────────────────────────

// searched + linked against the graph frozen at call start; slots[] are already appended & uploaded
// search half of a group of inserts against the graph as it stands (k_beam<BUILD>): per node and layer the first
// min(found, M_max) results → ws_sel / ws_nsel.  log_cap > 0 also records the link rows every search read.
static int build_search(mn_index *x, const int *slots, int nq, MnSearchArgs &a, int log_cap) {
    hipStream_t st = x->stream;
    const int fz_max = x->max_level;
    const int nlev = fz_max + 1;
    memset(&a, 0, sizeof(a));
    if (prepare_search_ws(x, nq, x->efc, a))
        return -1;
    // upper-layer bitmaps for batch nodes with level >= 1
    std::vector<int> upidx((size_t)nq, -1);
    int n_upper = 0;
    for (int j = 0; j < nq; j++)
        if (x->levels[slots[j]] >= 1 && fz_max >= 1)
            upidx[j] = n_upper++;
    a.bmu_words = bmu_words(x);
    if (n_upper) {
        size_t words = (size_t)n_upper * fz_max * a.bmu_words;
        if (x->ws_bmu.reserve(words, false, st)) return -1;
        HIPCHK(hipMemsetAsync(x->ws_bmu.p, 0, words * sizeof(unsigned), st));
    }
    a.bitmap_up = x->ws_bmu.p;
    if (x->ws_qslots.reserve((size_t)nq, false, st)) return -1;
    if (x->ws_upidx.reserve((size_t)nq, false, st)) return -1;
    if (x->ws_sel.reserve((size_t)nq * nlev * x->M_max0, false, st)) return -1;
    if (x->ws_nsel.reserve((size_t)nq * nlev, false, st)) return -1;
    HIPCHK(hipMemcpyAsync(x->ws_qslots.p, slots, (size_t)nq * sizeof(int), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(x->ws_upidx.p, upidx.data(), (size_t)nq * sizeof(int), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemsetAsync(x->ws_nsel.p, 0, (size_t)nq * nlev * sizeof(int), st));
    a.query_slots = x->ws_qslots.p;
    a.up_bm_index = x->ws_upidx.p;
    a.nq = nq;
    a.ef = x->efc;
    a.entry_slot = ht_find(x, x->entry_id);
    a.max_level = fz_max;
    a.sel = x->ws_sel.p;
    a.nsel = x->ws_nsel.p;
    a.nlev = nlev;
    if (log_cap > 0) {
        if (x->ws_readlog.reserve((size_t)nq * log_cap * MN_RLOG_INTS, false, st)) return -1;
        if (x->ws_nread.reserve((size_t)nq, false, st)) return -1;
        a.readlog = x->ws_readlog.p;
        a.readcap = log_cap;
        a.nread = x->ws_nread.p;
    }
    MnDevIndex v = dev_view(x);
    HIPCHK(hipEventRecord(x->ev0, st));
    x->last_on_host = false;
    mn_launch_search(v, a, true, st);
    HIPCHK(hipEventRecord(x->ev1, st));
    return 0;
}

// link half of a group of inserts: nq batch nodes (device array of their slots) with their selected lists; then the
// entry point / top layer update in batch order (src/hnsw_algo.c:660-663)
static int link_batch(mn_index *x, const std::vector<int> &slots, const int *d_slots, int nlev, const int *d_sel,
                      const int *d_nsel, mn_comm *c = nullptr) {
    hipStream_t st = x->stream;
    const int nq = (int)slots.size();
    MnDevIndex v = dev_view(x);
    const int max_tuples = nq * x->M_max0;
    if (x->lk_target.reserve((size_t)max_tuples, false, st)) return -1;
    if (x->lk_src.reserve((size_t)max_tuples, false, st)) return -1;
    if (x->lk_counters.reserve(4, false, st)) return -1;
    if (x->lk_count.reserve((size_t)x->d_ids.cap, false, st, 0)) return -1;
    if (x->lk_fill.reserve((size_t)x->d_ids.cap, false, st)) return -1;
    if (x->lk_binoff.reserve((size_t)x->d_ids.cap, false, st)) return -1;
    if (x->lk_touched.reserve((size_t)max_tuples, false, st)) return -1;
    if (x->lk_bins.reserve((size_t)max_tuples, false, st)) return -1;
    if (x->lk_newrows.reserve((size_t)max_tuples * std::max(x->W0, x->WU), false, st)) return -1;
    MnLinkArgs la;
    memset(&la, 0, sizeof(la));
    la.nq = nq;
    la.nlev = nlev;
    la.query_slots = d_slots;
    la.sel = d_sel;
    la.nsel = d_nsel;
    la.t_target = x->lk_target.p;
    la.t_src = x->lk_src.p;
    la.counters = x->lk_counters.p;
    la.count = x->lk_count.p;
    la.fill = x->lk_fill.p;
    la.binoff = x->lk_binoff.p;
    la.touched = x->lk_touched.p;
    la.bins = x->lk_bins.p;
    la.newrows = x->lk_newrows.p;
    const int world = c ? c->world : 1, rank = c ? c->rank : 0;
    if (world > 1) {
        // Jointly built graph: the replay of the reverse edges — the bulk of the link half — is divided over the ranks by
        // target (slot mod world).  Every rank runs the cheap forward half, so it knows every class's target count; it replays
        // its own class, the finished rows travel as {target, row} records in one all-gather per layer, and every replica
        // commits all of them: the same rows as a one-GPU build, whoever computed them.
        const int recsz = 1 + std::max(x->W0, x->WU);
        if (x->lk_rec.reserve((size_t)max_tuples * recsz, false, st) || x->lk_cls.reserve((size_t)world + 1, false, st))
            return -1;
        la.world = world;
        la.rank = rank;
        la.records = x->lk_rec.p;
        la.cls_count = x->lk_cls.p;
        la.rec_count = x->lk_cls.p + world;
        std::vector<int> cls((size_t)world);
        for (int l = 0; l < nlev; l++) {
            la.level = l;
            la.M_max = l == 0 ? x->M_max0 : x->M;
            const int mt = l == 0 ? max_tuples : nq * x->M;
            mn_launch_link_first(v, la, mt, st);
            int status = hipGetLastError() != hipSuccess ||
                         hipMemcpyAsync(cls.data(), x->lk_cls.p, (size_t)world * sizeof(int), hipMemcpyDeviceToHost, st) != hipSuccess ||
                         hipStreamSynchronize(st) != hipSuccess;
            int seg = 0;
            for (int r = 0; r < world && !status; r++)
                seg = std::max(seg, cls[(size_t)r]);
            if (!status && seg > 0 && x->lk_rec_all.reserve((size_t)world * seg * recsz, false, st))
                status = 1;
            int failed = -1;
            const int ag = mn_comm_agree(c, status, st, &failed); // (a rank that cannot go on says so before the collective)
            if (ag) {
                if (ag < 0)
                    set_err("mn_hnsw_build_shared: %s", mn_comm_last_error_str());
                else
                    set_err("mn_hnsw_build_shared: rank %d failed in the link step; all ranks stop", failed);
                return -1;
            }
            if (seg > 0) {
                int *mine = x->lk_rec_all.p + (size_t)rank * seg * recsz;
                if (cls[(size_t)rank] > 0)
                    HIPCHK(hipMemcpyAsync(mine, x->lk_rec.p, (size_t)cls[(size_t)rank] * recsz * sizeof(int), hipMemcpyDeviceToDevice, st));
                if (mn_comm_allgather_dev(c, mine, x->lk_rec_all.p, (size_t)seg * recsz * sizeof(int), st)) {
                    set_err("mn_hnsw_build_shared: %s", mn_comm_last_error_str());
                    return -1;
                }
            }
            mn_launch_link_commit_records(v, la, mt, x->lk_rec_all.p, seg, st);
        }
    } else {
        for (int l = 0; l < nlev; l++) {
            la.level = l;
            la.M_max = l == 0 ? x->M_max0 : x->M;
            int mt = l == 0 ? max_tuples : nq * x->M;
            mn_launch_link(v, la, mt, st);
        }
    }
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(x->ev2, st));
    HIPCHK(hipStreamSynchronize(st)); // (the searches' heap workspace was checked before this step: run_batch / batch_search)
    x->host_links_valid = false;
    for (int j = 0; j < nq; j++) {
        int lv = x->levels[slots[j]];
        if (lv > x->max_level) {
            x->entry_id = x->ids[slots[j]];
            x->max_level = lv;
        }
    }
    return 0;
}

static int run_batch(mn_index *x, const std::vector<int> &slots, bool *links_touched) {
    const int nq = (int)slots.size();
    *links_touched = false;
    if (nq == 0)
        return 0;
    const int nlev = x->max_level + 1;
    MnSearchArgs a;
    if (build_search(x, slots.data(), nq, a, 0))
        return -1;
    // the search half only reads the graph: a failure up to here leaves it untouched (the caller takes the nodes back)
    if (fetch_counters(x)) // synchronises
        return -1;
    if (x->last.last_n_overflow) {
        set_err("mn_hnsw_insert: %lld searches exceeded heap workspace", (long long)x->last.last_n_overflow);
        return -1;
    }
    *links_touched = true;
    x->bstats.search_ms += x->last.last_kernel_ms;
    x->bstats.n_dist += x->last.last_n_dist;
    x->bstats.n_expanded += x->last.last_n_expanded;
    x->bstats.batches++;
    x->bstats.nodes += nq;
    if (link_batch(x, slots, x->ws_qslots.p, nlev, x->ws_sel.p, x->ws_nsel.p))
        return -1;
    float ms = 0;
    if (hipEventElapsedTime(&ms, x->ev1, x->ev2) == hipSuccess)
        x->bstats.link_ms += ms;
    return 0;
}

static int run_sequential(mn_index *x, const std::vector<int> &slots) {
    hipStream_t st = x->stream;
    const int n = (int)slots.size();
    if (n == 0)
        return 0;
    if (mn_insert_seq_lds_bytes(dev_view(x)) > mn_lds_optin_limit()) { // (beyond 64 KB the launcher asks the device for the grant)
        set_err("mn_hnsw_insert: dimension %d with neighbour lists of up to %d entries does not fit the insert kernel's LDS", x->dim,
                std::max(x->W0, x->WU));
        return -1;
    }
    MnSearchArgs a;
    memset(&a, 0, sizeof(a));
    x->last_on_host = false;
    if (prepare_search_ws(x, 1, x->efc, a))
        return -1;
    if (x->ws_bmu.reserve((size_t)bmu_words(x), false, st)) return -1;
    if (x->ws_qslots.reserve((size_t)n, false, st)) return -1;
    if (x->ws_state.reserve(2, false, st)) return -1;
    int state[2] = {ht_find(x, x->entry_id), x->max_level};
    // one insert: inputs and outputs go through the pinned block (sized by sync_meta for this insert) and there is ONE wait
    unsigned char *pin = n == 1 && x->pin && x->pin_cap >= pin_insert_bytes(x) ? x->pin : nullptr;
    if (pin) {
        int *in = reinterpret_cast<int *>(pin + MN_PIN_IN);
        in[0] = slots[0];
        in[1] = state[0];
        in[2] = state[1];
        HIPCHK(hipMemcpyAsync(x->ws_qslots.p, in, sizeof(int), hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(x->ws_state.p, in + 1, 2 * sizeof(int), hipMemcpyHostToDevice, st));
    } else {
        HIPCHK(hipMemcpyAsync(x->ws_qslots.p, slots.data(), (size_t)n * sizeof(int), hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(x->ws_state.p, state, sizeof(state), hipMemcpyHostToDevice, st));
    }
    MnDevIndex v = dev_view(x);
    const bool logged = x->want_chlog && n == 1;
    x->want_chlog = false;
    if (logged && x->ws_chlog.reserve((size_t)1 + (size_t)MN_CHLOG_CAP * MN_CHLOG_INTS, false, st))
        return -1;
    HIPCHK(hipEventRecord(x->ev0, st));
    const int chunk = 1024; // keeps any one launch to about a second
    for (int pos = 0; pos < n; pos += chunk) {
        int m = std::min(chunk, n - pos);
        mn_launch_insert_seq(v, x->ws_qslots.p + pos, m, x->efc, x->ws_state.p, a.bitmap0, a.bm0_words, x->ws_bmu.p,
                             bmu_words(x), a.cand_ovf, a.cand_gcap, a.res_ovf, a.res_gcap, a.counters, st,
                             logged ? x->ws_chlog.p : nullptr, MN_CHLOG_CAP);
    }
    HIPCHK(hipEventRecord(x->ev1, st));
    HIPCHK(hipGetLastError());
    if (pin) {
        int *out = reinterpret_cast<int *>(pin + MN_PIN_OUT);
        const size_t log_ints = (size_t)1 + (size_t)MN_CHLOG_CAP * MN_CHLOG_INTS;
        HIPCHK(hipMemcpyAsync(out, x->ws_state.p, 2 * sizeof(int), hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(out + 2, x->ws_counters.p, 4 * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
        if (logged)
            HIPCHK(hipMemcpyAsync(pin + pin_log_off(x), x->ws_chlog.p, log_ints * sizeof(int), hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        state[0] = out[0];
        state[1] = out[1];
        unsigned long long c[8] = {0, 0, 0, 0, 0, 0, 0, 0}; // ([4] [5] stay zero: k_insert_seq walks every row with 4 lanes)
        memcpy(c, out + 2, 4 * sizeof(unsigned long long));
        last_from_counters(x, c, true);
        if (logged) {
            const int *lg = reinterpret_cast<const int *>(pin + pin_log_off(x));
            const int cnt = lg[0];
            x->h_chlog.assign(lg, lg + 1 + (size_t)(cnt > 0 && cnt <= MN_CHLOG_CAP ? cnt : 0) * MN_CHLOG_INTS);
        }
    } else {
        HIPCHK(hipMemcpyAsync(state, x->ws_state.p, sizeof(state), hipMemcpyDeviceToHost, st));
        if (logged) {
            x->h_chlog.assign((size_t)1 + (size_t)MN_CHLOG_CAP * MN_CHLOG_INTS, 0);
            HIPCHK(hipMemcpyAsync(x->h_chlog.data(), x->ws_chlog.p, x->h_chlog.size() * sizeof(int), hipMemcpyDeviceToHost, st));
        }
        if (fetch_counters(x))
            return -1;
    }
    if (x->last.last_n_overflow) {
        set_err("mn_hnsw_insert: heap workspace exceeded");
        return -1;
    }
    x->host_links_valid = false;
    x->entry_id = x->ids[state[0]];
    x->max_level = state[1];
    return 0;
}

// The same inserts, same order, same graph as run_sequential — by speculation (mn_spec.hip): windows of consecutive
// inserts are searched at once, then committed in order up to the first one whose search read a row that an earlier
// insert of the window rewrote; the next window starts there.
static int run_speculative(mn_index *x, const std::vector<int> &slots) {
    hipStream_t st = x->stream;
    const int n = (int)slots.size();
    const int LOG_CAP = 2048;
    if (x->d_stamp0.reserve((size_t)x->d_ids.cap, true, st, 0)) return -1;
    if (x->d_stampU.reserve((size_t)std::max(1, x->n_pool_rows) + 1, true, st, 0)) return -1;
    if (x->d_sidx0.reserve((size_t)x->d_ids.cap, false, st)) return -1; // (read only where the stamp is this window's)
    if (x->d_sidxU.reserve((size_t)std::max(1, x->n_pool_rows) + 1, false, st)) return -1;
    if (x->d_saved_rows.reserve((size_t)MN_SPEC_SAVE_CAP * 64, false, st)) return -1;
    if (x->ws_ncommit.reserve(1, false, st)) return -1;
    const bool trace = getenv("MN_SPEC_TRACE") != nullptr;
    if (trace) {
        if (x->d_spec_why.reserve(8, false, st)) return -1;
        HIPCHK(hipMemsetAsync(x->d_spec_why.p, 0, 8 * sizeof(int), st));
    }
    int window = 16, poor = 0;
    long long searched = 0, rounds = 0, plain = 0;
    double t_search = 0, t_commit = 0; // device ms (HIP events), reported under MN_SPEC_TRACE
    for (int pos = 0; pos < n;) {
        if (poor >= 8) {
            // a small index: nearly every search crosses the previous insert's rows, so windows commit one insert at a
            // time.  Run a stretch with the single-wavefront kernel, then try again (the index has grown meanwhile).
            const int m = std::min(512, n - pos);
            if (run_sequential(x, std::vector<int>(slots.begin() + pos, slots.begin() + pos + m)))
                return -1;
            pos += m;
            plain += m;
            poor = 4;
            continue;
        }
        int W = std::min(window, n - pos);
        // a node that raises the top layer becomes the entry point of everything after it (:660-663): it closes its window
        for (int k = 0; k < W; k++)
            if (x->levels[slots[pos + k]] > x->max_level) {
                W = k + 1;
                break;
            }
        MnSearchArgs a;
        if (build_search(x, slots.data() + pos, W, a, LOG_CAP))
            return -1;
        if (++x->spec_epoch == 0x7fffffff) { // epochs are compared for equality only: restart them before they wrap
            HIPCHK(hipMemsetAsync(x->d_stamp0.p, 0, x->d_stamp0.cap * sizeof(int), st));
            HIPCHK(hipMemsetAsync(x->d_stampU.p, 0, x->d_stampU.cap * sizeof(int), st));
            x->spec_epoch = 1;
        }
        MnDevIndex v = dev_view(x);
        // the link decisions of the whole window ahead of its commit (k_spec_prepare; MN_SPEC_AHEAD=0: decided inside the commit)
        const bool ahead = !(getenv("MN_SPEC_AHEAD") && atoi(getenv("MN_SPEC_AHEAD")) == 0) && v.W0 <= 64;
        if (ahead) {
            const size_t cells = (size_t)W * a.nlev * v.W0;
            if (x->d_pre_act.reserve(cells, false, st) || x->d_pre_cnt.reserve(cells, false, st) ||
                x->d_pre_row.reserve(cells * 64, false, st))
                return -1;
        }
        mn_launch_spec_commit(v, x->ws_qslots.p, W, a.nlev, x->ws_sel.p, x->ws_nsel.p, x->ws_readlog.p, LOG_CAP, x->ws_nread.p,
                              x->d_stamp0.p, x->d_stampU.p, x->d_sidx0.p, x->d_sidxU.p, x->d_saved_rows.p,
                              ahead ? x->d_pre_act.p : nullptr, x->d_pre_cnt.p, x->d_pre_row.p, trace ? x->d_spec_why.p : nullptr,
                              x->spec_epoch, x->ws_ncommit.p, st);
        HIPCHK(hipGetLastError());
        HIPCHK(hipEventRecord(x->ev2, st));
        int done = 0;
        HIPCHK(hipMemcpyAsync(&done, x->ws_ncommit.p, sizeof(int), hipMemcpyDeviceToHost, st));
        if (fetch_counters(x)) // synchronises
            return -1;
        {
            float ms = 0;
            t_search += x->last.last_kernel_ms;
            if (hipEventElapsedTime(&ms, x->ev1, x->ev2) == hipSuccess)
                t_commit += ms;
        }
        if (x->last.last_n_overflow) {
            set_err("mn_hnsw_insert: heap workspace exceeded");
            return -1;
        }
        if (done < 1 || done > W) {
            set_err("mn_hnsw_insert: speculative commit returned %d of %d", done, W);
            return -1;
        }
        for (int k = 0; k < done; k++) { // entry point / top layer in insertion order (:660-663)
            int lv = x->levels[slots[pos + k]];
            if (lv > x->max_level) {
                x->entry_id = x->ids[slots[pos + k]];
                x->max_level = lv;
            }
        }
        searched += W;
        rounds++;
        pos += done;
        poor = done <= 1 && W > 1 ? poor + 1 : 0;
        // A window's searches run side by side and a search is one latency-bound wavefront, so a wider window costs
        // bandwidth, not time; searches beyond the committed prefix are simply repeated.  Keep it a few times the prefix.
        window = done == W ? std::min(128, window * 2) : std::max(16, std::min(128, 3 * done)); // (≤ 128: one workgroup each, k_beam_coop)
    }
    x->host_links_valid = false;
    x->last_spec_searched = searched;
    if (trace) {
        int why[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        HIPCHK(hipMemcpy(why, x->d_spec_why.p, sizeof(why), hipMemcpyDeviceToHost));
        fprintf(stderr, "[mn_spec] windows ended by: log overflow %d, > 64 rewritten rows %d, a row with the log's defaults %d, an old list "
                        "not kept %d, a removed neighbour the search could have pushed %d, an added node it would have pushed %d, a "
                        "greedy step that would have gone elsewhere %d; committed whole %d\n", why[1], why[2], why[3], why[4], why[5],
                why[6], why[0], why[7]);
    }
    if (trace)
        fprintf(stderr, "[mn_spec] %d inserts: %lld rounds (%.1f committed per round), %lld searches, %lld by k_insert_seq; device ms "
                        "per round: search %.2f commit %.2f\n", n, rounds, rounds ? (double)(n - plain) / rounds : 0.0, searched, plain,
                rounds ? t_search / rounds : 0.0, rounds ? t_commit / rounds : 0.0);
    return 0;
}

#define MN_BUILD_STAGE_ONLY 100 // internal: add the nodes, leave search + link to mn_hnsw_batch_search / _link

static int insert_impl(mn_index *x, const int64_t *ids, const float *vectors, int64_t n, int mode, bool src_on_device = false) {
    if (use_device(x))
        return -1;
    if (n <= 0)
        return 0;
    // duplicates against the index and inside the call (src/hnsw_algo.c:522)
    {
        std::vector<int64_t> sorted(ids, ids + n);
        std::sort(sorted.begin(), sorted.end());
        for (int64_t i = 1; i < n; i++)
            if (sorted[i] == sorted[i - 1]) {
                set_err("mn_hnsw_insert: duplicate id %lld in batch", (long long)sorted[i]);
                return -1;
            }
        for (int64_t i = 0; i < n; i++)
            if (ht_find(x, ids[i]) >= 0) {
                set_err("mn_hnsw_insert: duplicate id %lld", (long long)ids[i]);
                return -1;
            }
    }
    {
        const int64_t f = first_table_full(x, n);
        if (f >= 0) {
            // the reference: random_level() is drawn, ht_insert fails, hnsw_insert returns -1 (src/hnsw_algo.c:532-540)
            if (n == 1)
                (void)random_level(x);
            set_err("mn_hnsw_insert: node table full (%d entries incl. soft-deleted nodes; the table grows on the live count only)",
                    x->ht_cap);
            return -1;
        }
    }
    if (push_links(x))
        return -1;
    const int first = x->n_slots;
    InsertUndo undo;
    undo.first = first;
    undo.node_count = x->node_count;
    undo.max_level = x->max_level;
    undo.n_pool_rows = x->n_pool_rows;
    undo.rng = x->rng_state;
    undo.entry_id = x->entry_id;
    bool links_touched = false, any_rest = false;
    try {
    std::vector<int> slots((size_t)n);
    for (int64_t i = 0; i < n; i++) {
        if (x->node_count * 10 > x->ht_cap * 7) { // :527
            if (undo.grew_at < 0) {
                undo.grew_at = x->n_slots;
                undo.old_ht = x->ht;
                undo.old_cap = x->ht_cap;
            }
            ht_grow(x);
        }
        int level = random_level(x); // :532
        slots[i] = host_add_node(x, ids[i], level, 0);
        if (slots[i] < 0) { // (first_table_full rules this out)
            undo_insert(x, undo);
            set_err("mn_hnsw_insert: node table insert failed for id %lld", (long long)ids[i]);
            return -1;
        }
        x->node_count++;
    }
    if (sync_meta(x) || upload_vectors(x, first, vectors, (int)n, src_on_device)) {
        undo_insert(x, undo);
        return -1;
    }
    HIPCHK(hipMemsetAsync(x->d_dirty.p + first, 1, (size_t)n, x->stream)); // new nodes are always persisted
    size_t pos = 0;
    if (x->entry_id == -1) { // :544-548 first node just becomes the entry point
        x->entry_id = ids[0];
        x->max_level = x->levels[slots[0]];
        pos = 1;
        // -1 is the reference's "no entry point" marker AND a legal rowid: after inserting rowid -1 into an empty index
        // the reference still believes it is empty and the next insert becomes the entry point too, unlinked
        // (one-at-a-time semantics only; found by scripts/fuzz_parity.py)
        while (mode == MN_BUILD_SEQUENTIAL && x->entry_id == -1 && pos < (size_t)n) {
            x->entry_id = ids[pos];
            x->max_level = x->levels[slots[pos]];
            pos++;
        }
    }
    std::vector<int> rest(slots.begin() + pos, slots.end());
    if (mode == MN_BUILD_STAGE_ONLY) { // mn_hnsw_batch_stage: the caller drives search and link itself
        x->staged.swap(rest);
        return 0;
    }
    int rc;
    any_rest = !rest.empty();
    links_touched = true; // the exact modes edit rows in place from the first insert on
    if (mode == MN_BUILD_SEQUENTIAL) {
        // same result either way; speculation pays once several inserts are queued (MN_SPECULATE=0 turns it off)
        const char *sp = getenv("MN_SPECULATE");
        const bool spec_on = !(sp && atoi(sp) == 0);
        // (k_spec_commit stages ≤ 64 targets of ≤ 64 links, on rows that never outgrew M_max)
        if (spec_on && rest.size() >= 4 && x->W0 <= 64 && x->W0 == x->M_max0 && x->WU == x->M)
            rc = run_speculative(x, rest);
        else
            rc = run_sequential(x, rest);
    } else {
        rc = run_batch(x, rest, &links_touched);
    }
    if (rc != 0) {
        // "nothing inserted on -1": take the nodes back while the graph is still as it was; past that point the rows of
        // existing nodes may already name the new slots, and the index refuses further use instead of serving them
        if (!links_touched)
            undo_insert(x, undo);
        else if (!rest.empty())
            x->broken = true;
    }
    return rc;
    } catch (...) {
        // the same promise when host memory ran out half way (std::bad_alloc out of a table or a staging vector): nothing
        // inserted while the graph is as it was, an unusable index past that point; the C-ABI's barrier reports it
        if (!links_touched)
            undo_insert(x, undo);
        else if (any_rest)
            x->broken = true;
        throw;
    }
}

// The persist set of src/hnsw_vtab.c:755-768, accumulated over any number of inserts: every new node and
// every node that was a neighbour of a new node when it was linked.  Reading it clears it.
extern "C" int64_t mn_hnsw_take_dirty(mn_index *x, int64_t *ids, int64_t cap) try {
    if (use_device(x))
        return -1;
    if (x->n_slots == 0 || !x->d_dirty.p)
        return 0;
    const size_t n = std::min((size_t)x->n_slots, x->d_dirty.cap);
    std::vector<unsigned char> h(n);
    HIPCHK(hipStreamSynchronize(x->stream));
    HIPCHK(hipMemcpy(h.data(), x->d_dirty.p, n, hipMemcpyDeviceToHost));
    int64_t cnt = 0;
    for (size_t s = 0; s < n; s++)
        cnt += h[s] != 0;
    if (cnt > cap)
        return cnt; // nothing cleared: call again with room for cnt ids
    int64_t o = 0;
    for (size_t s = 0; s < n; s++)
        if (h[s]) {
            ids[o++] = x->ids[s];
            if (s < x->h_stale.size() && x->h_stale[s]) { // the caller rewrites this node whole
                x->h_stale[s] = 0;
                x->n_stale--;
            }
        }
    HIPCHK(hipMemset(x->d_dirty.p, 0, n));
    return cnt;
} MN_GUARD_END(set_err, MN_NOTHING, -1)

extern "C" int mn_hnsw_insert(mn_index *x, int64_t id, const float *vector) try {
    return insert_impl(x, &id, vector, 1, MN_BUILD_SEQUENTIAL);
} MN_GUARD_END(set_err, MN_NOTHING, -1)

extern "C" int mn_hnsw_insert_batch(mn_index *x, const int64_t *ids, const float *vectors, int64_t n, int mode) try {
    return insert_impl(x, ids, vectors, n, mode);
} MN_GUARD_END(set_err, MN_NOTHING, -1)

// hnsw_insert (src/hnsw_algo.c:520-666) that also says WHICH edges it added and removed: the caller's persistence
// (src/hnsw_vtab.c:755-776 rewrites the "{t}_edges" rows of the new node and of every neighbour — ≈ 1 100 rows per insert) can
// then touch only the ≈ 100 rows that changed.  *n_log = entries written (op 1: edge src -> dst added at `level` with
// `distance`; op 2: edge src -> dst removed), or -1 when the log cannot describe this insert (more than `cap` changes, a
// neighbour list wider than 64 links, or a touched node whose lists an earlier mn_hnsw_delete edited — the reference never
// persisted those edits, so only a whole rewrite of that node matches it): the persist set (mn_hnsw_take_dirty) is then
// still complete.  With a valid log the persist set is emptied — the caller has everything.  Same graph, same return
// convention as mn_hnsw_insert.
extern "C" int mn_hnsw_insert_logged(mn_index *x, int64_t id, const float *vector, mn_edge_change *log, int cap, int *n_log) try {
    *n_log = -1;
    if (use_device(x))
        return -1;
    const int was_slots = x->n_slots;
    x->want_chlog = true;
    x->h_chlog.clear();
    const int rc = insert_impl(x, &id, vector, 1, MN_BUILD_SEQUENTIAL);
    x->want_chlog = false;
    if (rc != 0)
        return rc;
    if (x->n_slots == was_slots + 1 && x->h_chlog.empty()) { // first node of an empty index: no search, no edges
        *n_log = 0;
    } else if (!x->h_chlog.empty() && x->h_chlog[0] >= 0 && x->h_chlog[0] <= cap) {
        const int n = x->h_chlog[0];
        bool stale = false; // touched = the new node's selected neighbours = dst of its own "added" entries
        for (int i = 0; i < n && x->n_stale > 0 && !stale; i++) {
            const int *e = x->h_chlog.data() + 1 + (size_t)i * MN_CHLOG_INTS;
            stale = e[0] == 1 && (size_t)e[3] < x->h_stale.size() && x->h_stale[e[3]];
        }
        for (int i = 0; i < n && !stale; i++) {
            const int *e = x->h_chlog.data() + 1 + (size_t)i * MN_CHLOG_INTS;
            log[i].op = e[0];
            log[i].src = x->ids[e[1]];
            log[i].level = e[2];
            log[i].dst = x->ids[e[3]];
            memcpy(&log[i].distance, &e[4], sizeof(float));
        }
        if (!stale)
            *n_log = n;
    }
    if (*n_log >= 0 && x->d_dirty.p && x->n_slots > 0) // (the log replaces the persist set for this insert)
        HIPCHK(hipMemsetAsync(x->d_dirty.p, 0, std::min((size_t)x->n_slots, x->d_dirty.cap), x->stream));
    return 0;
} MN_GUARD_END(set_err, MN_NOTHING, -1)

// The caller's edge-by-edge copy of the graph no longer matches the index — for the n given nodes, or (ids == NULL) for every
// node present now (its transaction rolled back): logged inserts report -1 for every insert that touches such a node, until
// the node has gone through the persist set (a whole rewrite).  Unknown ids are ignored.
extern "C" int mn_hnsw_log_invalidate(mn_index *x, const int64_t *ids, int64_t n) try {
    if (!x)
        return -1;
    if (!ids) {
        x->h_stale.assign((size_t)x->n_slots, 1);
        x->n_stale = x->n_slots;
        return 0;
    }
    for (int64_t i = 0; i < n; i++) {
        const int s = ht_find(x, ids[i]);
        if (s >= 0)
            mark_stale(x, s);
    }
    return 0;
} MN_GUARD_END(set_err, MN_NOTHING, -1)

static int build_impl(mn_index *x, const int64_t *ids, const float *vectors, int64_t n, int grow_div, int max_batch,
                      bool src_on_device) {
    if (grow_div <= 0)
        grow_div = 16;
    if (max_batch <= 0)
        max_batch = 8192;
    if (!getenv("MN_BUILD_NO_RESERVE"))
        x->slot_hint = (int64_t)x->n_slots + n; // the slot-indexed device tables are allocated once, at their final size
    int64_t pos = 0;
    while (pos < n) {
        int64_t b = std::max<int64_t>(1, x->node_count / grow_div);
        b = std::min<int64_t>(b, max_batch);
        b = std::min<int64_t>(b, n - pos);
        if (insert_impl(x, ids + pos, vectors + (size_t)pos * x->dim, b, MN_BUILD_BATCHED, src_on_device))
            return -1;
        pos += b;
    }
    return 0;
}

extern "C" int mn_hnsw_build(mn_index *x, const int64_t *ids, const float *vectors, int64_t n, int grow_div,
                             int max_batch) try {
    return build_impl(x, ids, vectors, n, grow_div, max_batch, false);
} MN_GUARD_END(set_err, if (x) x->broken = true, -1)

// the same build from rows that are already in HBM on the index's device ([n][dim] f32, e.g. the embeddings a Node2Vec run
// has just normalised: mn_node2vec_train_into): same batches, same graph as mn_hnsw_build on a host copy of those rows
extern "C" int mn_hnsw_build_dev(mn_index *x, const int64_t *ids, const float *d_vectors, int64_t n, int grow_div,
                                 int max_batch) try {
    return build_impl(x, ids, d_vectors, n, grow_div, max_batch, true);
} MN_GUARD_END(set_err, if (x) x->broken = true, -1)

// ── one batch of the batch-synchronous build in three steps, so that the search half can be split over several GPUs
//    that each hold a replica of the index (sqlite-muninn_amd/parallel.py build_distributed) ──
#define MN_STAGE_CHECK(x)                                                       \
    if (use_device(x))                                                          \
        return -1;

extern "C" int mn_hnsw_batch_stage(mn_index *x, const int64_t *ids, const float *vectors, int64_t n) try {
    MN_STAGE_CHECK(x)
    if (!x->staged.empty()) {
        set_err("mn_hnsw_batch_stage: the previous batch was not linked");
        return -1;
    }
    if (insert_impl(x, ids, vectors, n, MN_BUILD_STAGE_ONLY))
        return -1;
    const int m = (int)x->staged.size();
    if (m) {
        if (x->d_staged.reserve((size_t)m, false, x->stream)) return -1;
        HIPCHK(hipMemcpy(x->d_staged.p, x->staged.data(), (size_t)m * sizeof(int), hipMemcpyHostToDevice));
    }
    return m;
} MN_GUARD_END(set_err, if (x) x->broken = true, -1)

extern "C" int mn_hnsw_batch_dims(mn_index *x, int *nlev, int *row_width) try {
    *nlev = x->max_level + 1;
    *row_width = x->M_max0;
    return 0;
} MN_GUARD_END(set_err, MN_NOTHING, -1)

extern "C" int mn_hnsw_batch_search(mn_index *x, int lo, int hi, int *d_sel, int *d_nsel) try {
    MN_STAGE_CHECK(x)
    const int m = (int)x->staged.size();
    if (lo < 0 || hi > m || lo > hi) {
        set_err("mn_hnsw_batch_search: bad range [%d, %d) of %d staged nodes", lo, hi, m);
        return -1;
    }
    if (hi == lo)
        return 0;
    const int nlev = x->max_level + 1;
    MnSearchArgs a;
    if (build_search(x, x->staged.data() + lo, hi - lo, a, 0))
        return -1;
    const size_t row = (size_t)nlev * x->M_max0;
    HIPCHK(hipMemcpyAsync(d_sel + (size_t)lo * row, x->ws_sel.p, (size_t)(hi - lo) * row * sizeof(int), hipMemcpyDeviceToDevice,
                          x->stream));
    HIPCHK(hipMemcpyAsync(d_nsel + (size_t)lo * nlev, x->ws_nsel.p, (size_t)(hi - lo) * nlev * sizeof(int), hipMemcpyDeviceToDevice,
                          x->stream));
    if (fetch_counters(x)) // synchronises
        return -1;
    if (x->last.last_n_overflow) {
        set_err("mn_hnsw_batch_search: %lld searches exceeded heap workspace", (long long)x->last.last_n_overflow);
        return -1;
    }
    return 0;
} MN_GUARD_END(set_err, if (x) x->broken = true, -1)

static int batch_link_impl(mn_index *x, const int *d_sel, const int *d_nsel, mn_comm *c) {
    MN_STAGE_CHECK(x)
    std::vector<int> slots;
    slots.swap(x->staged);
    if (slots.empty())
        return 0;
    return link_batch(x, slots, x->d_staged.p, x->max_level + 1, d_sel, d_nsel, c);
}
extern "C" int mn_hnsw_batch_link(mn_index *x, const int *d_sel, const int *d_nsel) try {
    return batch_link_impl(x, d_sel, d_nsel, nullptr);
} MN_GUARD_END(set_err, if (x) x->broken = true, -1)

// ───────────────────────── multi-GPU: the jointly built graph ─────────────────────────

extern "C" int mn_hnsw_build_shared(mn_index *x, mn_comm *c, const int64_t *ids, const float *vectors, int64_t n, int grow_div,
                                    int max_batch, int min_split) try {
    MN_STAGE_CHECK(x)
    if (grow_div <= 0)
        grow_div = 16;
    if (max_batch <= 0)
        max_batch = 8192;
    if (min_split <= 0)
        min_split = 256;
    const int world = c ? c->world : 1, rank = c ? c->rank : 0;
    hipStream_t st = x->stream;
    if (!getenv("MN_BUILD_NO_RESERVE"))
        x->slot_hint = (int64_t)x->n_slots + n;
    int64_t pos = 0;
    while (pos < n) {
        int64_t b = std::max<int64_t>(1, x->node_count / grow_div); // the batches of mn_hnsw_build
        b = std::min<int64_t>(b, max_batch);
        b = std::min<int64_t>(b, n - pos);
        // A rank whose local step fails (staging, workspace, its slice of the searches: overflow, out of memory) may not simply
        // return: its peers are in — or about to enter — the batch's all-gather and would wait for ever.  Every rank finishes
        // its local step, the ranks exchange one status word, and all of them fail together (mn_comm_agree).
        int status = 0;
        const int m = mn_hnsw_batch_stage(x, ids + pos, vectors + (size_t)pos * x->dim, b);
        if (m < 0)
            status = 1;
        if (const char *fi = getenv("MN_FAULT_INJECT")) { // test hook: "build_shared:<rank>:<first id position of the batch>"
            int fr = -1;
            long long fp = -1;
            if (sscanf(fi, "build_shared:%d:%lld", &fr, &fp) == 2 && fr == rank && fp >= pos && fp < pos + b && !status) {
                set_err("injected failure (MN_FAULT_INJECT)");
                status = 1;
            }
        }
        pos += b;
        const int nlev = x->max_level + 1, w0 = x->M_max0;
        const bool split = world > 1 && m >= min_split;
        const int per = split ? (m + world - 1) / world : std::max(m, 0);
        const int rows = split ? per * world : std::max(m, 0);
        const size_t row_sel = (size_t)nlev * w0;
        if (!status && m > 0) {
            if (x->sh_sel.reserve((size_t)rows * row_sel, false, st) || x->sh_nsel.reserve((size_t)rows * nlev, false, st) ||
                hipMemsetAsync(x->sh_sel.p, 0xFF, (size_t)rows * row_sel * sizeof(int), st) != hipSuccess ||
                hipMemsetAsync(x->sh_nsel.p, 0, (size_t)rows * nlev * sizeof(int), st) != hipSuccess) {
                status = 1;
            } else {
                const int lo = split ? std::min(m, rank * per) : 0, hi = split ? std::min(m, rank * per + per) : m;
                // from here on the batch's nodes are in the host tables but not linked: a failure must not leave a half-built
                // index in use
                if (mn_hnsw_batch_search(x, lo, hi, x->sh_sel.p, x->sh_nsel.p)) { // this rank's slice of the batch's searches
                    x->broken = true;
                    status = 1;
                }
            }
        }
        if (world > 1) {
            int failed = -1;
            const std::string mine = status ? std::string(mn_last_error()) : std::string();
            const int ag = mn_comm_agree(c, status, st, &failed);
            if (ag) {
                if (ag < 0)
                    set_err("mn_hnsw_build_shared: %s", mn_comm_last_error_str());
                else if (failed == rank)
                    set_err("mn_hnsw_build_shared: rank %d failed: %s", rank, mine.c_str());
                else
                    set_err("mn_hnsw_build_shared: rank %d failed in this batch; all ranks stop", failed);
                x->broken = true;
                return -1;
            }
        } else if (status) {
            return -1;
        }
        if (m == 0)
            continue;
        if (split) { // in place: rank r's rows already sit at r * per
            if (mn_comm_allgather_dev(c, x->sh_sel.p + (size_t)rank * per * row_sel, x->sh_sel.p, (size_t)per * row_sel * sizeof(int), st) ||
                mn_comm_allgather_dev(c, x->sh_nsel.p + (size_t)rank * per * nlev, x->sh_nsel.p, (size_t)per * nlev * sizeof(int), st)) {
                set_err("mn_hnsw_build_shared: %s", mn_comm_last_error_str());
                x->broken = true;
                return -1;
            }
        }
        // every replica links the whole batch; with a divided batch the reverse edges' replay is divided too (link_batch)
        if (batch_link_impl(x, x->sh_sel.p, x->sh_nsel.p, split && !getenv("MN_SHARED_LINK_REPLICATED") ? c : nullptr)) {
            x->broken = true;
            return -1;
        }
    }
    return 0;
} MN_GUARD_END(set_err, if (x) x->broken = true, -1)
