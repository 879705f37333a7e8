// mn_index.hip — host side of libmuninn_hip.so: the C-ABI of include/muninn_hip.h over a
// device-resident HNSW index.  No CPU compute path exists here: distances, searches and link
// updates are HIP kernels (mn_kernels.hip, mn_build.hip); the host only keeps the id→slot table,
// per-node metadata, the level RNG (src/hnsw_algo.c:19-30,240-248) and the cold delete path.
// This unit: the handle, the id table and host metadata, the host mirror of the links, delete, load, export and the measurement
// hooks.  The search drivers are in mn_index_search.hip, the insert and build drivers in mn_index_insert.hip; what the three
// share is declared in mn_index_int.hpp.
#include "mn_index_int.hpp"

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <unordered_map>
#include <mutex>

#define MN_MAX_M 512        // longest supported M (lists of 2M + 1 entries are pruned in LDS)
#define MN_MAX_ROW 2048     // longest neighbour list a row may grow to through deletes / loads (same LDS budget)

static thread_local std::string g_err;

void set_err(const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    mn_vformat(g_err, fmt, ap);
    va_end(ap);
}

// ── host allocations of this library: countable, and the n-th one can be made to fail (test hook of the exception barrier,
//    mn_guard.hpp).  The linker's export map (exports.map: mn_* only) keeps the replacement private to this shared object: it
//    serves the new-expressions compiled into it (std::vector, std::string bodies instantiated here) and nothing else in the
//    process. ──
#include <atomic>
static std::atomic<long long> g_alloc_count{0}, g_alloc_fail_at{0};
static inline void *mn_counted_alloc(size_t n) {
    const long long c = g_alloc_count.fetch_add(1, std::memory_order_relaxed) + 1;
    if (c == g_alloc_fail_at.load(std::memory_order_relaxed))
        throw std::bad_alloc();
    void *p = malloc(n ? n : 1);
    if (!p)
        throw std::bad_alloc();
    return p;
}
void *operator new(size_t n) { return mn_counted_alloc(n); }
void *operator new[](size_t n) { return mn_counted_alloc(n); }
void operator delete(void *p) noexcept { free(p); }
void operator delete[](void *p) noexcept { free(p); }
void operator delete(void *p, size_t) noexcept { free(p); }
void operator delete[](void *p, size_t) noexcept { free(p); }
extern "C" long long mn_debug_fault_alloc(long long nth) {
    g_alloc_fail_at.store(nth > 0 ? nth : 0, std::memory_order_relaxed);
    return g_alloc_count.exchange(0, std::memory_order_relaxed);
}

// ───────────────────────── small host helpers ─────────────────────────

static unsigned xorshift32(unsigned *state) { // src/hnsw_algo.c:19-26
    unsigned x = *state;
    x ^= x << 13;
    x ^= x >> 17;
    x ^= x << 5;
    *state = x;
    return x;
}

int random_level(mn_index *x) { // src/hnsw_algo.c:240-248
    double r = (double)xorshift32(&x->rng_state) / (double)0xFFFFFFFFu;
    if (r == 0.0)
        r = 1e-10;
    int level = (int)(-log(r) * x->level_mult);
    if (level >= 32)
        level = 31;
    return level;
}

static int ht_hash(int64_t id, int cap) { // src/hnsw_algo.c:38-47
    uint64_t h = (uint64_t)id;
    h ^= h >> 33;
    h *= 0xff51afd7ed558ccdULL;
    h ^= h >> 33;
    h *= 0xc4ceb9fe1a85ec53ULL;
    h ^= h >> 33;
    return (int)(h & (uint64_t)(cap - 1));
}

int ht_find(const mn_index *x, int64_t id) {
    int s = ht_hash(id, x->ht_cap);
    for (int i = 0; i < x->ht_cap; i++) {
        int p = (s + i) & (x->ht_cap - 1);
        if (x->ht[p] < 0)
            return -1;
        if (x->ids[x->ht[p]] == id)
            return x->ht[p];
    }
    return -1;
}

static int ht_put(std::vector<int> &t, int cap, const std::vector<int64_t> &ids, int slot) {
    int s = ht_hash(ids[slot], cap);
    for (int i = 0; i < cap; i++) {
        int p = (s + i) & (cap - 1);
        if (t[p] < 0) {
            t[p] = slot;
            return 0;
        }
        if (ids[t[p]] == ids[slot])
            return -1;
    }
    return -1;
}

void ht_grow(mn_index *x) { // src/hnsw_algo.c:76-91: rehash in old-table order
    int nc = x->ht_cap * 2;
    std::vector<int> nt((size_t)nc, -1);
    for (int i = 0; i < x->ht_cap; i++)
        if (x->ht[i] >= 0)
            ht_put(nt, nc, x->ids, x->ht[i]);
    x->ht.swap(nt);
    x->ht_cap = nc;
}

// The reference grows its table on the LIVE count (src/hnsw_algo.c:527) while soft-deleted nodes keep their entries, so
// delete + insert churn can fill it; ht_insert then fails ("table full", :61-74) and hnsw_insert returns -1.  Index of the
// first of n inserts that would hit that, or -1.
int64_t first_table_full(const mn_index *x, int64_t n) {
    long long cap = x->ht_cap, live = x->node_count, occ = x->n_slots;
    for (int64_t i = 0; i < n; i++) {
        if (live * 10 > cap * 7)
            cap *= 2;
        if (occ >= cap)
            return i;
        live++;
        occ++;
    }
    return -1;
}

static void ht_erase_newest(std::vector<int> &t, int cap, const std::vector<int64_t> &ids, int slot) {
    // entries are erased newest first, so each one is the last link of its probe chain: clearing it restores the table
    int s = ht_hash(ids[slot], cap);
    for (int i = 0; i < cap; i++) {
        int p = (s + i) & (cap - 1);
        if (t[p] == slot) {
            t[p] = -1;
            return;
        }
    }
}

void undo_insert(mn_index *x, InsertUndo &u) {
    int hi = x->n_slots;
    if (u.grew_at >= 0) {
        x->ht.swap(u.old_ht);
        x->ht_cap = u.old_cap;
        hi = u.grew_at;
    }
    for (int s = hi - 1; s >= u.first; s--)
        ht_erase_newest(x->ht, x->ht_cap, x->ids, s);
    x->ids.resize((size_t)u.first);
    x->levels.resize((size_t)u.first);
    x->deleted.resize((size_t)u.first);
    x->up_off.resize((size_t)u.first);
    x->n_slots = u.first;
    x->n_pool_rows = u.n_pool_rows;
    x->node_count = u.node_count;
    x->rng_state = u.rng;
    x->entry_id = u.entry_id;
    x->max_level = u.max_level;
    x->meta_uploaded = std::min(x->meta_uploaded, u.first);
    x->staged.clear();
    if (x->host_links_valid) {
        x->h_links0.resize((size_t)x->n_slots * x->W0);
        x->h_links_up.resize((size_t)x->n_pool_rows * x->WU);
    }
}

int use_device(mn_index *x) {
    if (x->broken) {
        set_err("index unusable: an earlier insert failed after it had begun to rewrite neighbour rows");
        return -1;
    }
    HIPCHK(hipSetDevice(x->device));
    return 0;
}

MnDevIndex dev_view(mn_index *x) {
    MnDevIndex v;
    v.vectors = x->d_vectors.p;
    v.norms = x->d_norms.p;
    v.links0 = x->d_links0.p;
    v.links_up = x->d_links_up.p;
    v.up_off = x->d_up_off.p;
    v.levels = x->d_levels.p;
    v.deleted = x->d_deleted.p;
    v.dirty = x->d_dirty.p;
    v.ids = x->d_ids.p;
    v.dim = x->dim;
    v.ld = x->ld;
    v.metric = x->metric;
    v.order = x->order;
    v.W0 = x->W0;
    v.WU = x->WU;
    v.M0 = x->M_max0;
    v.MU = x->M;
    v.WX = std::max(x->W0, x->WU);
    v.n_slots = x->n_slots;
    v.n_pool_rows = x->n_pool_rows;
    v.has_deleted = x->n_deleted > 0;
    v.vec_lo = x->d_vec_lo.p;
    v.lo_meta = x->d_lo_meta.p;
    return v;
}

// append a node to the host tables (node_create + ht_insert); returns slot
int host_add_node(mn_index *x, int64_t id, int level, int deleted) {
    int s = x->n_slots;
    x->ids.push_back(id);
    x->levels.push_back((signed char)level);
    x->deleted.push_back((unsigned char)deleted);
    if (level > 0) {
        x->up_off.push_back(x->n_pool_rows);
        x->n_pool_rows += level;
    } else {
        x->up_off.push_back(-1);
    }
    x->n_slots++;
    if (ht_put(x->ht, x->ht_cap, x->ids, s) != 0) {
        x->ids.pop_back();
        x->levels.pop_back();
        x->deleted.pop_back();
        if (level > 0)
            x->n_pool_rows -= level;
        x->up_off.pop_back();
        x->n_slots--;
        return -1;
    }
    if (x->host_links_valid) {
        x->h_links0.resize((size_t)x->n_slots * x->W0, -1);
        x->h_links_up.resize((size_t)x->n_pool_rows * x->WU, -1);
    }
    return s;
}

// the index's pinned host block (staging of one insert, mailbox of a small search), at least `need` bytes; nullptr on failure
unsigned char *pin_reserve(mn_index *x, size_t need) {
    if (need <= x->pin_cap)
        return x->pin;
    if (hipStreamSynchronize(x->stream) != hipSuccess) // (copies out of the old block may still be queued)
        return nullptr;
    if (x->pin)
        (void)hipHostFree(x->pin);
    x->pin = nullptr;
    x->pin_cap = 0;
    void *p = nullptr;
    if (hipHostMalloc(&p, need * 2, hipHostMallocDefault) != hipSuccess)
        return nullptr;
    x->pin = (unsigned char *)p;
    x->pin_cap = need * 2;
    return x->pin;
}

int sync_meta(mn_index *x) {
    hipStream_t st = x->stream;
    size_t ns = (size_t)x->n_slots;
    size_t hs = std::max(ns, (size_t)x->slot_hint); // a bulk build has announced its final slot count
    if (x->d_vectors.reserve(ns * x->ld, true, st, -1, hs * x->ld)) return -1;
    if (x->d_norms.reserve(ns, true, st, -1, hs)) return -1;
    if (mn_lo_enabled(x->ld)) {
        if (x->d_vec_lo.reserve(ns * mn_lo_row_words(x->ld), true, st, -1, hs * mn_lo_row_words(x->ld))) return -1;
        if (x->d_lo_meta.reserve(ns, true, st, -1, hs)) return -1;
    }
    if (x->d_links0.reserve(ns * x->W0, true, st, 0xFF, hs * x->W0)) return -1;
    if (x->d_links_up.reserve((size_t)std::max(1, x->n_pool_rows) * x->WU, true, st, 0xFF)) return -1;
    if (x->d_up_off.reserve(ns, true, st, -1, hs)) return -1;
    if (x->d_levels.reserve(ns, true, st, -1, hs)) return -1;
    if (x->d_deleted.reserve(ns, true, st, -1, hs)) return -1;
    if (x->d_dirty.reserve(ns, true, st, 0, hs)) return -1;
    if (x->d_ids.reserve(ns, true, st, -1, hs)) return -1;
    int a = x->meta_uploaded, n = x->n_slots - a;
    unsigned char *pin = n == 1 ? pin_reserve(x, pin_insert_bytes(x)) : nullptr;
    if (n == 1 && pin) { // one insert: staged in the pinned block — four truly asynchronous copies, nothing to wait for
        HIPCHK(hipStreamSynchronize(st)); // (whoever starts writing into the block waits for its previous user; idle as a rule)
        int *pi = reinterpret_cast<int *>(pin + MN_PIN_META);
        pi[0] = x->up_off[a];
        reinterpret_cast<unsigned char *>(pi + 1)[0] = (unsigned char)x->levels[a];
        reinterpret_cast<unsigned char *>(pi + 2)[0] = x->deleted[a];
        memcpy(pi + 4, &x->ids[a], sizeof(long long));
        HIPCHK(hipMemcpyAsync(x->d_up_off.p + a, pi, sizeof(int), hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(x->d_levels.p + a, pi + 1, 1, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(x->d_deleted.p + a, pi + 2, 1, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(x->d_ids.p + a, pi + 4, sizeof(long long), hipMemcpyHostToDevice, st));
        x->meta_uploaded = x->n_slots;
    } else if (n > 0) {
        HIPCHK(hipMemcpyAsync(x->d_up_off.p + a, x->up_off.data() + a, (size_t)n * sizeof(int), hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(x->d_levels.p + a, x->levels.data() + a, (size_t)n, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(x->d_deleted.p + a, x->deleted.data() + a, (size_t)n, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(x->d_ids.p + a, x->ids.data() + a, (size_t)n * sizeof(long long), hipMemcpyHostToDevice, st));
        HIPCHK(hipStreamSynchronize(st)); // host vectors may be reallocated by later appends
        x->meta_uploaded = x->n_slots;
    }
    if (!x->load_vecs.empty()) { // vectors of loaded nodes (mn_hnsw_load_node): one upload for the lot
        std::vector<float> v;
        v.swap(x->load_vecs);
        const int first = x->load_first;
        x->load_first = -1;
        if (upload_vectors(x, first, v.data(), (int)(v.size() / (size_t)x->dim)))
            return -1;
    }
    return 0;
}

// what is derived from rows [first, first + n) once they are in place: norms (cosine) and the coded shadow, one launch
static void prep_rows(mn_index *x, int first, int n) {
    mn_launch_prep_rows(dev_view(x), first, n, x->metric == MN_METRIC_COSINE ? x->d_norms.p : nullptr, x->d_vec_lo.p,
                        x->d_lo_meta.p, x->stream);
}

int upload_vectors(mn_index *x, int first, const float *vecs, int n, bool src_on_device) {
    hipStream_t st = x->stream;
    // (src_on_device: the rows are already in HBM — mn_hnsw_build_dev — and never visit the host)
    const hipMemcpyKind kind = src_on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
    if (n == 1 && !src_on_device && x->pin && x->pin_cap >= pin_insert_bytes(x)) { // (sync_meta has just sized the block)
        float *pv = reinterpret_cast<float *>(x->pin + MN_PIN_VEC);
        memcpy(pv, vecs, (size_t)x->dim * sizeof(float));
        for (int i = x->dim; i < x->ld; i++)
            pv[i] = 0.0f;
        HIPCHK(hipMemcpyAsync(x->d_vectors.p + (size_t)first * x->ld, pv, (size_t)x->ld * sizeof(float), hipMemcpyHostToDevice, st));
        prep_rows(x, first, 1);
        return 0; // the insert's own synchronisation covers the copy
    }
    if (x->ld == x->dim) {
        HIPCHK(hipMemcpyAsync(x->d_vectors.p + (size_t)first * x->ld, vecs, (size_t)n * x->dim * sizeof(float), kind, st));
    } else {
        HIPCHK(hipMemsetAsync(x->d_vectors.p + (size_t)first * x->ld, 0, (size_t)n * x->ld * sizeof(float), st));
        HIPCHK(hipMemcpy2DAsync(x->d_vectors.p + (size_t)first * x->ld, (size_t)x->ld * sizeof(float), vecs,
                                (size_t)x->dim * sizeof(float), (size_t)x->dim * sizeof(float), (size_t)n, kind, st));
    }
    prep_rows(x, first, n);
    HIPCHK(hipStreamSynchronize(st));
    return 0;
}

static size_t d_row_off(const mn_index *x, int slot, int level) { // element offset of a row inside d_links0 / d_links_up
    return level == 0 ? (size_t)slot * x->W0 : ((size_t)x->up_off[slot] + (level - 1)) * x->WU;
}

int pull_links(mn_index *x) {
    if (x->host_links_valid)
        return 0;
    x->h_links0.assign((size_t)x->n_slots * x->W0, -1);
    x->h_links_up.assign((size_t)x->n_pool_rows * x->WU, -1);
    const size_t n0 = std::min(x->h_links0.size(), x->d_links0.cap), nu = std::min(x->h_links_up.size(), x->d_links_up.cap);
    if (n0)
        HIPCHK(hipMemcpyAsync(x->h_links0.data(), x->d_links0.p, n0 * sizeof(int), hipMemcpyDeviceToHost, x->stream));
    if (nu)
        HIPCHK(hipMemcpyAsync(x->h_links_up.data(), x->d_links_up.p, nu * sizeof(int), hipMemcpyDeviceToHost, x->stream));
    HIPCHK(hipStreamSynchronize(x->stream));
    x->host_links_valid = true;
    x->dev_links_stale = false;
    x->dev_links_all = false;
    x->h_dirty_rows.clear();
    return 0;
}

static int *h_row(mn_index *x, int slot, int level, int *W);

int push_links(mn_index *x) {
    if (!x->dev_links_stale)
        return 0;
    if (sync_meta(x))
        return -1;
    if (x->dev_links_all) {
        if (x->n_slots)
            HIPCHK(hipMemcpyAsync(x->d_links0.p, x->h_links0.data(), x->h_links0.size() * sizeof(int), hipMemcpyHostToDevice,
                                  x->stream));
        if (x->n_pool_rows)
            HIPCHK(hipMemcpyAsync(x->d_links_up.p, x->h_links_up.data(), x->h_links_up.size() * sizeof(int),
                                  hipMemcpyHostToDevice, x->stream));
    } else {
        for (const auto &r : x->h_dirty_rows) { // a delete edits a few dozen rows: send those, not the table
            int W;
            const int *row = h_row(x, r.first, r.second, &W);
            int *dst = (r.second == 0 ? x->d_links0.p : x->d_links_up.p) + d_row_off(x, r.first, r.second);
            HIPCHK(hipMemcpyAsync(dst, row, (size_t)W * sizeof(int), hipMemcpyHostToDevice, x->stream));
        }
    }
    HIPCHK(hipStreamSynchronize(x->stream));
    x->dev_links_stale = false;
    x->dev_links_all = false;
    x->h_dirty_rows.clear();
    return 0;
}

static int *h_row(mn_index *x, int slot, int level, int *W) {
    if (level == 0) {
        *W = x->W0;
        return x->h_links0.data() + (size_t)slot * x->W0;
    }
    *W = x->WU;
    return x->h_links_up.data() + ((size_t)x->up_off[slot] + (level - 1)) * x->WU;
}

// Give the rows of one kind (layer 0, or the layers above) a longer stride.  Needs the full mirror; the device copy is
// dropped and rebuilt from it at the next push (fresh buffers, so that rows of future slots read as empty).
static int restride(mn_index *x, bool layer0, int newW) {
    if (pull_links(x))
        return -1;
    std::vector<int> &h = layer0 ? x->h_links0 : x->h_links_up;
    const int oldW = layer0 ? x->W0 : x->WU;
    const size_t rows = layer0 ? (size_t)x->n_slots : (size_t)x->n_pool_rows;
    std::vector<int> nh(rows * (size_t)newW, -1);
    for (size_t r = 0; r < rows; r++)
        memcpy(nh.data() + r * newW, h.data() + r * oldW, (size_t)oldW * sizeof(int));
    h.swap(nh);
    (layer0 ? x->W0 : x->WU) = newW;
    (void)hipStreamSynchronize(x->stream);
    (layer0 ? x->d_links0 : x->d_links_up).release();
    x->dev_links_stale = true;
    x->dev_links_all = true;
    return 0;
}

static int h_row_count(const int *row, int W) {
    int n = 0;
    while (n < W && row[n] >= 0)
        n++;
    return n;
}

// ───────────────────────── library ─────────────────────────

extern "C" int mn_abi_version(void) { return MN_ABI_VERSION; }
extern "C" const char *mn_last_error(void) { return g_err.c_str(); }

extern "C" int mn_device_count(void) try {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess)
        return 0;
    int ok = 0;
    for (int i = 0; i < n; i++) {
        hipDeviceProp_t p;
        if (hipGetDeviceProperties(&p, i) == hipSuccess && strncmp(p.gcnArchName, "gfx950", 6) == 0)
            ok++;
    }
    return ok;
} MN_GUARD_END(set_err, MN_NOTHING, -1)

extern "C" int mn_vec_parse_metric(const char *name, int *out) { // src/vec_math.c:192-204
    if (!name || !out)
        return -1;
    if (strcmp(name, "l2") == 0) {
        *out = MN_METRIC_L2;
        return 0;
    }
    if (strcmp(name, "cosine") == 0) {
        *out = MN_METRIC_COSINE;
        return 0;
    }
    if (strcmp(name, "inner_product") == 0) {
        *out = MN_METRIC_INNER_PRODUCT;
        return 0;
    }
    return -1;
}

extern "C" int mn_vec_dist_batch(int metric, int order, const float *query, const float *rows, int64_t n, int dim,
                                 float *out) try {
    if (mn_device_count() <= 0) {
        set_err("mn_vec_dist_batch: no gfx950 device");
        return -1;
    }
    if (n <= 0)
        return 0;
    int ld = (dim + 3) & ~3;
    IndexBuf<float> dq, dr, dout; // released on every path
    if (dq.reserve((size_t)dim, false, nullptr) || dr.reserve((size_t)n * ld, false, nullptr) || dout.reserve((size_t)n, false, nullptr))
        return -1;
    HIPCHK(hipMemcpy(dq.p, query, (size_t)dim * sizeof(float), hipMemcpyHostToDevice));
    HIPCHK(hipMemset(dr.p, 0, (size_t)n * ld * sizeof(float)));
    HIPCHK(hipMemcpy2D(dr.p, (size_t)ld * sizeof(float), rows, (size_t)dim * sizeof(float), (size_t)dim * sizeof(float),
                       (size_t)n, hipMemcpyHostToDevice));
    if (mn_launch_dist_batch(metric, order, dq.p, dr.p, n, dim, ld, dout.p, nullptr)) {
        set_err("mn_vec_dist_batch: dim=%d needs %zu bytes of LDS, this device grants %zu", dim, mn_dist_batch_lds_bytes(ld),
                mn_lds_optin_limit());
        return -1;
    }
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(out, dout.p, (size_t)n * sizeof(float), hipMemcpyDeviceToHost));
    return 0;
} MN_GUARD_END(set_err, MN_NOTHING, -1)

// ───────────────────────── create / destroy ─────────────────────────

// Whether an index of rows of ld floats and this M fits the LDS of every kernel it launches, by the launchers' own formulas: 64 KB
// where a launcher never asks for more, what the device grants where it does (k_insert_seq).  The optional parts (distance tiles,
// precomputed prunes, visited bitmaps) are added only where they fit and are left out.  The batched link step is taken at the
// build's default batch of 8192 nodes (its bitmap grows with the batch, not with the row).
static bool ld_fits(int ld, int M, size_t optin) {
    const size_t lim = 64 * 1024;
    MnDevIndex v;
    memset(&v, 0, sizeof(v));
    v.ld = ld;
    v.M0 = v.W0 = 2 * M; // src/hnsw_algo.c:188
    v.MU = v.WU = M;
    v.WX = 2 * M;
#ifdef MN_SSE_TILE_PATH
    const bool tile = true;
#else
    const bool tile = false;
#endif
    return mn_search_lds_bytes(ld, tile) <= lim && mn_coop_lds_bytes(ld, tile) <= lim && // k_beam, k_beam_coop
           mn_insert_seq_lds_bytes(v) <= optin &&                                          // k_insert_seq (asks for the grant)
           (v.W0 > 64 || mn_spec_commit_min_lds_bytes(ld) <= lim) &&                     // k_spec_commit (M <= 32 only)
           mn_link_reverse_lds_bytes(ld, v.WX, 8192) <= lim &&                            // k_link_reverse
           mn_bruteforce_lds_bytes(ld) <= lim && mn_row_lds_bytes(ld) <= lim;             // k_bruteforce, k_prep_rows, k_edge_rows
}
// the largest dimension an index with this M can have on this device (every formula grows with ld); 0: none
static int max_dim(int M, int device) {
    int cur = 0;
    (void)hipGetDevice(&cur);
    if (cur != device)
        (void)hipSetDevice(device);
    const size_t optin = mn_lds_optin_limit();
    if (cur != device)
        (void)hipSetDevice(cur);
    int lo = 0, hi = 1 << 20; // ld = 4 lo fits (or lo = 0), ld = 4 hi does not
    while (hi - lo > 1) {
        const int mid = lo + (hi - lo) / 2;
        (ld_fits(4 * mid, M, optin) ? lo : hi) = mid;
    }
    return 4 * lo;
}
extern "C" int mn_hnsw_max_dim(int M, int device) try {
    int ndev = 0;
    if (M < 2 || M > MN_MAX_M || hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) {
        set_err("mn_hnsw_max_dim: bad parameters or no HIP device %d", device);
        return -1;
    }
    return max_dim(M, device);
} MN_GUARD_END(set_err, MN_NOTHING, -1)

extern "C" mn_index *mn_hnsw_create_on(int dim, int metric, int M, int ef_construction, int device) try {
    if (dim <= 0 || M < 2 || ef_construction < 1 || metric < 0 || metric > 2) {
        set_err("mn_hnsw_create: bad parameters");
        return nullptr;
    }
    if (M > MN_MAX_M) { // the reference has no upper bound; here a list (2M + 1 entries, three LDS arrays) must fit a workgroup's LDS
        set_err("mn_hnsw_create: M=%d exceeds this build's limit of %d", M, MN_MAX_M);
        return nullptr;
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) {
        set_err("mn_hnsw_create: HIP device %d not available (no CPU fallback)", device);
        return nullptr;
    }
    // the reference has no upper bound; here every kernel stages rows of the index in LDS
    if (const int lim = max_dim(M, device); dim > lim) {
        set_err("mn_hnsw_create: dim=%d exceeds this build's limit of %d for M=%d on device %d", dim, lim, M, device);
        return nullptr;
    }
    mn_index *x = new mn_index();
    x->device = device;
    x->dim = dim;
    x->ld = (dim + 3) & ~3;
    x->metric = metric;
    x->M = M;
    x->M_max0 = 2 * M; // src/hnsw_algo.c:188
    x->W0 = x->M_max0;
    x->WU = M;
    x->efc = ef_construction;
    x->level_mult = 1.0 / log((double)M); // :192
    x->ht.assign(256, -1);                // :197
    if (hipSetDevice(device) != hipSuccess || hipStreamCreateWithFlags(&x->stream, hipStreamNonBlocking) != hipSuccess ||
        hipEventCreate(&x->ev0) != hipSuccess || hipEventCreate(&x->ev1) != hipSuccess || hipEventCreate(&x->ev2) != hipSuccess) {
        set_err("mn_hnsw_create: cannot create HIP stream/events on device %d", device);
        delete x;
        return nullptr;
    }
    { // once per process and device: the kernels' code objects are loaded now, not under the first query (MN_LAZY_MODULES=1: as before)
        static std::mutex mu;
        static unsigned long long touched = 0;
        std::lock_guard<std::mutex> lk(mu);
        if (device < 64 && !(touched >> device & 1ull) && !getenv("MN_LAZY_MODULES")) {
            touched |= 1ull << device;
            mn_module_touch_kernels();
            mn_module_touch_seq();
            mn_module_touch_spec();
            mn_module_touch_build();
        }
    }
    return x;
} MN_GUARD_END(set_err, MN_NOTHING, nullptr)

extern "C" mn_index *mn_hnsw_create(int dim, int metric, int M, int ef_construction) try {
    return mn_hnsw_create_on(dim, metric, M, ef_construction, 0);
} MN_GUARD_END(set_err, MN_NOTHING, nullptr)

extern "C" void mn_hnsw_destroy(mn_index *x) {
    if (!x)
        return;
    (void)hipSetDevice(x->device);
    if (x->stream)
        (void)hipStreamSynchronize(x->stream);
    if (x->pin)
        (void)hipHostFree(x->pin);
    // the device buffers (DevBuf members), then the events, then the stream (MnStreamEvents): an index is deleted only with its
    // device selected, as here and in mn_hnsw_create_on
    delete x;
}

extern "C" void mn_hnsw_seed_rng(mn_index *x, unsigned seed) { x->rng_state = seed ? seed : 1; }

extern "C" int mn_hnsw_set_order(mn_index *x, int order) try {
    if (x->n_slots > 0) {
        set_err("mn_hnsw_set_order: index not empty");
        return -1;
    }
    if (order != MN_ORDER_SSE && order != MN_ORDER_WAVE)
        return -1;
    x->order = order;
    return 0;
} MN_GUARD_END(set_err, if (x) x->broken = true, -1)

void mark_stale(mn_index *x, int slot) {
    if (x->h_stale.size() < (size_t)x->n_slots)
        x->h_stale.resize((size_t)x->n_slots, 0);
    if (!x->h_stale[slot]) {
        x->h_stale[slot] = 1;
        x->n_stale++;
    }
}

extern "C" int mn_hnsw_device(mn_index *x) { return x->device; }

// ───────────────────────── delete (cold path, host-side list surgery) ─────────────────────────
// hnsw_delete edits the lists of the deleted node's neighbours only (a few dozen rows).  Those rows are worked on as
// plain growable lists — the reference's node_add_neighbor grows a list without bound (src/hnsw_algo.c:142-163) — read
// from the host mirror when it is current and otherwise row by row from HBM, and written back the same way.  Only when
// a list ends up longer than the row stride is the table re-strided (rare: reconnection under heavy deletion at tiny M).

struct RowEdit {
    mn_index *x;
    std::unordered_map<unsigned long long, std::vector<int>> rows;
    std::vector<unsigned long long> modified;
    static unsigned long long key(int slot, int level) { return ((unsigned long long)level << 32) | (unsigned)slot; }
    std::vector<int> *get(int slot, int level) {
        const unsigned long long k = key(slot, level);
        auto it = rows.find(k);
        if (it != rows.end())
            return &it->second;
        const int W = level == 0 ? x->W0 : x->WU;
        std::vector<int> buf((size_t)W, -1);
        if (x->host_links_valid) {
            int w2;
            memcpy(buf.data(), h_row(x, slot, level, &w2), (size_t)W * sizeof(int));
        } else {
            const int *src = (level == 0 ? x->d_links0.p : x->d_links_up.p) + d_row_off(x, slot, level);
            if (hipMemcpy(buf.data(), src, (size_t)W * sizeof(int), hipMemcpyDeviceToHost) != hipSuccess)
                return nullptr;
        }
        buf.resize((size_t)h_row_count(buf.data(), W));
        return &(rows[k] = std::move(buf));
    }
    void touch(int slot, int level) { modified.push_back(key(slot, level)); }
};

static int grown_stride(int W, int need) { // a little headroom, so that a run of deletes does not re-stride every time
    int nw = std::max(need, W + std::max(16, W / 2));
    return (nw + 15) & ~15;
}

extern "C" int mn_hnsw_delete(mn_index *x, int64_t id) try { // src/hnsw_algo.c:717-805
    if (use_device(x))
        return -1;
    const int s = ht_find(x, id);
    if (s < 0 || x->deleted[s])
        return -1;
    if (push_links(x) || sync_meta(x)) // rows are read from whichever copy is current
        return -1;
    HIPCHK(hipStreamSynchronize(x->stream));
    RowEdit ed{x, {}, {}};
    const int min_conn = x->M / 2;
    auto live_at = [&](int n, int l) { return !x->deleted[n] && l <= x->levels[n]; };
    // (the reference flags the node deleted first, :722; nothing below looks at that flag for s itself)
    for (int l = 0; l <= x->levels[s]; l++) {
        std::vector<int> *own = ed.get(s, l);
        if (!own) {
            set_err("mn_hnsw_delete: cannot read neighbour rows");
            return -1;
        }
        const std::vector<int> former(*own); // :731-738
        const int nc = (int)former.size();
        for (int i = 0; i < nc; i++) { // :741-746 node_remove_neighbor: swap with last (:166-177)
            const int nb = former[i];
            if (x->deleted[nb] || l > x->levels[nb])
                continue;
            std::vector<int> *r = ed.get(nb, l);
            if (!r)
                return -1;
            for (size_t k = 0; k < r->size(); k++)
                if ((*r)[k] == s) {
                    (*r)[k] = r->back();
                    r->pop_back();
                    ed.touch(nb, l);
                    break;
                }
        }
        for (int i = 0; i < nc; i++) { // :750-785 reconnect neighbours left with fewer than M/2 links
            const int orphan = former[i];
            if (!live_at(orphan, l))
                continue;
            std::vector<int> *orow = ed.get(orphan, l);
            if (!orow)
                return -1;
            if ((int)orow->size() >= min_conn)
                continue;
            for (int j = 0; j < nc && (int)orow->size() < min_conn; j++) {
                if (i == j)
                    continue;
                const int cand = former[j];
                if (!live_at(cand, l))
                    continue;
                if (std::find(orow->begin(), orow->end(), cand) != orow->end())
                    continue;
                orow->push_back(cand); // node_add_neighbor(orphan, l, cand): not present (checked above)
                ed.touch(orphan, l);
                std::vector<int> *crow = ed.get(cand, l);
                if (!crow)
                    return -1;
                orow = ed.get(orphan, l); // (the map may have rehashed)
                if (std::find(crow->begin(), crow->end(), orphan) == crow->end()) { // node_add_neighbor skips duplicates (:147-150)
                    crow->push_back(orphan);
                    ed.touch(cand, l);
                }
            }
        }
    }
    // longest list per kind of row → does the table need a longer stride?
    int need0 = 0, needU = 0;
    for (unsigned long long k : ed.modified) {
        const int len = (int)ed.rows[k].size();
        ((k >> 32) == 0 ? need0 : needU) = std::max((k >> 32) == 0 ? need0 : needU, len);
    }
    if (std::max(need0, needU) > MN_MAX_ROW) {
        set_err("mn_hnsw_delete: a neighbour list would grow to %d entries (limit %d)", std::max(need0, needU), MN_MAX_ROW);
        return -1;
    }
    if (need0 > x->W0 && restride(x, true, grown_stride(x->W0, need0)))
        return -1;
    if (needU > x->WU && restride(x, false, grown_stride(x->WU, needU)))
        return -1;
    std::sort(ed.modified.begin(), ed.modified.end());
    ed.modified.erase(std::unique(ed.modified.begin(), ed.modified.end()), ed.modified.end());
    for (unsigned long long k : ed.modified) {
        const int slot = (int)(k & 0xffffffffu), level = (int)(k >> 32);
        const std::vector<int> &list = ed.rows[k];
        const int W = level == 0 ? x->W0 : x->WU;
        mark_stale(x, slot);
        std::vector<int> padded((size_t)W, -1);
        std::copy(list.begin(), list.end(), padded.begin());
        if (x->host_links_valid) {
            int w2;
            memcpy(h_row(x, slot, level, &w2), padded.data(), (size_t)W * sizeof(int));
            if (!x->dev_links_all)
                x->h_dirty_rows.push_back({slot, level});
            x->dev_links_stale = true;
        } else {
            int *dst = (level == 0 ? x->d_links0.p : x->d_links_up.p) + d_row_off(x, slot, level);
            HIPCHK(hipMemcpy(dst, padded.data(), (size_t)W * sizeof(int), hipMemcpyHostToDevice));
        }
    }
    x->deleted[s] = 1; // :722-723
    x->node_count--;
    x->n_deleted++;
    if (x->entry_id == id) { // :790-802 scan in hash-table order, strict >
        x->entry_id = -1;
        x->max_level = -1;
        for (int i = 0; i < x->ht_cap; i++) {
            int t = x->ht[i];
            if (t >= 0 && !x->deleted[t] && x->levels[t] > x->max_level) {
                x->max_level = x->levels[t];
                x->entry_id = x->ids[t];
            }
        }
    }
    if (s < x->meta_uploaded)
        HIPCHK(hipMemcpy(x->d_deleted.p + s, &x->deleted[s], 1, hipMemcpyHostToDevice));
    return 0;
} MN_GUARD_END(set_err, if (x) x->broken = true, -1)

// ───────────────────────── inspection / load ─────────────────────────

extern "C" int mn_hnsw_get_vector(mn_index *x, int64_t id, float *out) try {
    if (use_device(x))
        return -1;
    int s = ht_find(x, id);
    if (s < 0 || x->deleted[s])
        return -1;
    if (!x->load_vecs.empty() && sync_meta(x))
        return -1;
    HIPCHK(hipMemcpy(out, x->d_vectors.p + (size_t)s * x->ld, (size_t)x->dim * sizeof(float), hipMemcpyDeviceToHost));
    return 0;
} MN_GUARD_END(set_err, MN_NOTHING, -1)

extern "C" int mn_hnsw_node_count(mn_index *x) { return x->node_count; }
extern "C" int64_t mn_hnsw_entry_point(mn_index *x) { return x->entry_id; }
extern "C" int mn_hnsw_max_level(mn_index *x) { return x->max_level; }
extern "C" int mn_hnsw_node_level(mn_index *x, int64_t id) try {
    int s = ht_find(x, id);
    return s < 0 ? -1 : x->levels[s];
} MN_GUARD_END(set_err, MN_NOTHING, -1)
extern "C" int mn_hnsw_node_deleted(mn_index *x, int64_t id) try {
    int s = ht_find(x, id);
    return s < 0 ? -1 : x->deleted[s];
} MN_GUARD_END(set_err, MN_NOTHING, -1)

extern "C" int mn_hnsw_neighbors(mn_index *x, int64_t id, int level, int64_t *out, int cap) try {
    if (use_device(x))
        return -1;
    int s = ht_find(x, id);
    if (s < 0 || level > x->levels[s])
        return -1;
    int W = level == 0 ? x->W0 : x->WU;
    std::vector<int> tmp;
    const int *row;
    if (x->host_links_valid) {
        row = h_row(x, s, level, &W);
    } else { // one row straight from HBM: do not pull the whole graph for a point read
        tmp.resize((size_t)W);
        HIPCHK(hipStreamSynchronize(x->stream));
        HIPCHK(hipMemcpy(tmp.data(), (level == 0 ? x->d_links0.p : x->d_links_up.p) + d_row_off(x, s, level),
                         (size_t)W * sizeof(int), hipMemcpyDeviceToHost));
        row = tmp.data();
    }
    int n = h_row_count(row, W);
    for (int i = 0; i < n && i < cap; i++)
        out[i] = x->ids[row[i]];
    return n;
} MN_GUARD_END(set_err, MN_NOTHING, -1)

extern "C" int mn_hnsw_load_node(mn_index *x, int64_t id, const float *vector, int level, int deleted) try {
    if (use_device(x))
        return -1;
    if (level < 0 || level >= 32)
        return -1;
    if (pull_links(x))
        return -1;
    if (x->node_count * 10 > x->ht_cap * 7) // src/hnsw_vtab.c:304-306
        ht_grow(x);
    int s = host_add_node(x, id, level, deleted);
    if (s < 0) {
        // Table full (it grows on the LIVE count while soft-deleted rows keep their entries): the reference's load loop
        // ignores ht_insert's failure and carries on without the node (src/hnsw_vtab.c:316); so does this one.
        // A duplicate id takes the same path there.
        return 1;
    }
    if (!deleted)
        x->node_count++;
    else
        x->n_deleted++;
    // host only: the vector waits for one bulk upload (sync_meta) instead of a copy + two synchronisations per row
    if (x->load_vecs.empty())
        x->load_first = s;
    x->load_vecs.insert(x->load_vecs.end(), vector, vector + x->dim);
    x->dev_links_stale = true; // new (empty) rows of the mirror
    x->dev_links_all = true;
    if (x->load_vecs.size() * sizeof(float) >= (256u << 20))
        return sync_meta(x);
    return 0;
} MN_GUARD_END(set_err, if (x) x->broken = true, -1)

extern "C" int mn_hnsw_load_neighbors(mn_index *x, int64_t id, int level, const int64_t *nbrs, int n) try {
    if (use_device(x))
        return -1;
    int s = ht_find(x, id);
    if (s < 0 || level > x->levels[s])
        return -1;
    if (pull_links(x))
        return -1;
    for (int i = 0; i < n; i++) {
        int t = ht_find(x, nbrs[i]);
        if (t < 0) { // (a row the caller holds and the index does not: a whole rewrite of s is what removes it)
            mark_stale(x, s);
            continue;
        }
        int W;
        int *row = h_row(x, s, level, &W);
        int cnt = h_row_count(row, W);
        bool present = false; // node_add_neighbor (src/hnsw_algo.c:142-163): no duplicates, grows as needed
        for (int k = 0; k < cnt; k++)
            present |= row[k] == t;
        if (present)
            continue;
        if (cnt >= W) { // a list longer than M_max (left by deletes in the database that is being loaded)
            if (cnt + 1 > MN_MAX_ROW) {
                set_err("mn_hnsw_load_neighbors: more than %d neighbours at level %d", MN_MAX_ROW, level);
                return -1;
            }
            if (restride(x, level == 0, grown_stride(W, cnt + 1)))
                return -1;
            row = h_row(x, s, level, &W);
        }
        row[cnt] = t;
    }
    x->dev_links_stale = true;
    x->dev_links_all = true;
    return 0;
} MN_GUARD_END(set_err, if (x) x->broken = true, -1)

extern "C" int mn_hnsw_set_entry(mn_index *x, int64_t entry, int max_level) try {
    x->entry_id = entry;
    x->max_level = max_level;
    return 0;
} MN_GUARD_END(set_err, if (x) x->broken = true, -1)

// ───────────────────────── bulk export ─────────────────────────

extern "C" int mn_hnsw_slot_count(mn_index *x) { return x->n_slots; }

extern "C" int mn_hnsw_export_nodes(mn_index *x, int64_t *ids, int *levels, int *deleted) try {
    for (int s = 0; s < x->n_slots; s++) {
        ids[s] = x->ids[s];
        levels[s] = x->levels[s];
        deleted[s] = x->deleted[s];
    }
    return 0;
} MN_GUARD_END(set_err, MN_NOTHING, -1)

extern "C" int mn_hnsw_export_vectors(mn_index *x, float *out) try {
    if (use_device(x))
        return -1;
    if (x->n_slots == 0)
        return 0;
    if (sync_meta(x))
        return -1;
    HIPCHK(hipStreamSynchronize(x->stream));
    HIPCHK(hipMemcpy2D(out, (size_t)x->dim * sizeof(float), x->d_vectors.p, (size_t)x->ld * sizeof(float),
                       (size_t)x->dim * sizeof(float), (size_t)x->n_slots, hipMemcpyDeviceToHost));
    return 0;
} MN_GUARD_END(set_err, MN_NOTHING, -1)

extern "C" int mn_hnsw_row_width(mn_index *x, int level) { return level == 0 ? x->W0 : x->WU; }

extern "C" int mn_hnsw_export_links(mn_index *x, int level, int *out, int *width) try {
    if (use_device(x))
        return -1;
    if (pull_links(x))
        return -1;
    const int W = level == 0 ? x->W0 : x->WU;
    *width = W;
    for (int s = 0; s < x->n_slots; s++) {
        int *dst = out + (size_t)s * W;
        if (level > x->levels[s]) {
            for (int i = 0; i < W; i++)
                dst[i] = -1;
        } else {
            int w2;
            const int *row = h_row(x, s, level, &w2);
            memcpy(dst, row, (size_t)W * sizeof(int));
        }
    }
    return 0;
} MN_GUARD_END(set_err, MN_NOTHING, -1)

extern "C" int64_t mn_hnsw_edges_of(mn_index *x, const int64_t *ids, int n, int64_t *out_src, int64_t *out_dst,
                                    int *out_level, float *out_dist, int64_t cap) try {
    if (use_device(x))
        return -1;
    if (push_links(x) || sync_meta(x))
        return -1;
    std::vector<int> rs, rl;
    for (int i = 0; i < n; i++) {
        int s = ht_find(x, ids[i]);
        if (s < 0) {
            set_err("mn_hnsw_edges_of: unknown id %lld", (long long)ids[i]);
            return -1;
        }
        for (int l = 0; l <= x->levels[s]; l++) {
            rs.push_back(s);
            rl.push_back(l);
        }
    }
    const int R = (int)rs.size();
    if (R == 0)
        return 0;
    hipStream_t st = x->stream;
    const int W0 = std::max(x->W0, x->WU); // rows of either kind are written with the common stride WX
    if (x->er_slot.reserve((size_t)R, false, st)) return -1;
    if (x->er_level.reserve((size_t)R, false, st)) return -1;
    if (x->er_nbr.reserve((size_t)R * W0, false, st)) return -1;
    if (x->er_dist.reserve((size_t)R * W0, false, st)) return -1;
    HIPCHK(hipMemcpyAsync(x->er_slot.p, rs.data(), (size_t)R * sizeof(int), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(x->er_level.p, rl.data(), (size_t)R * sizeof(int), hipMemcpyHostToDevice, st));
    mn_launch_edge_rows(dev_view(x), x->er_slot.p, x->er_level.p, R, x->er_nbr.p, x->er_dist.p, st);
    HIPCHK(hipGetLastError());
    std::vector<int> nbr((size_t)R * W0);
    std::vector<float> dist((size_t)R * W0);
    HIPCHK(hipMemcpyAsync(nbr.data(), x->er_nbr.p, nbr.size() * sizeof(int), hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(dist.data(), x->er_dist.p, dist.size() * sizeof(float), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    int64_t ne = 0;
    for (int r = 0; r < R; r++)
        for (int i = 0; i < W0; i++) {
            int t = nbr[(size_t)r * W0 + i];
            if (t < 0)
                break;
            if (ne < cap) {
                out_src[ne] = x->ids[rs[r]];
                out_dst[ne] = x->ids[t];
                out_level[ne] = rl[r];
                out_dist[ne] = dist[(size_t)r * W0 + i];
            }
            ne++;
        }
    return ne;
} MN_GUARD_END(set_err, MN_NOTHING, -1)

// ───────────────────────── measurement hooks ─────────────────────────

extern "C" int mn_hnsw_build_stats(mn_index *x, mn_build_stats *out, int reset) try {
    *out = x->bstats;
    if (reset)
        x->bstats = {0, 0, 0, 0, 0, 0};
    return 0;
} MN_GUARD_END(set_err, MN_NOTHING, -1)

extern "C" int mn_hnsw_last_launch(mn_index *x, mn_launch_stats *out) try {
    if (use_device(x))
        return -1;
    if (!x->last_on_host && fetch_counters(x)) // (a lone query's counters came back with its answer)
        return -1;
    *out = x->last;
    return 0;
} MN_GUARD_END(set_err, MN_NOTHING, -1)

extern "C" void *mn_dev_malloc(mn_index *x, size_t bytes) try {
    void *p = nullptr;
    if (hipSetDevice(x->device) != hipSuccess || hipMalloc(&p, bytes) != hipSuccess) {
        set_err("mn_dev_malloc(%zu) failed", bytes);
        return nullptr;
    }
    return p;
} MN_GUARD_END(set_err, MN_NOTHING, nullptr)
extern "C" void mn_dev_free(mn_index *x, void *p) {
    (void)hipSetDevice(x->device);
    (void)hipFree(p);
}
extern "C" int mn_dev_upload(mn_index *x, void *dst, const void *src, size_t bytes) try {
    if (use_device(x))
        return -1;
    HIPCHK(hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice));
    return 0;
} MN_GUARD_END(set_err, MN_NOTHING, -1)
extern "C" int mn_dev_download(mn_index *x, void *dst, const void *src, size_t bytes) try {
    if (use_device(x))
        return -1;
    HIPCHK(hipStreamSynchronize(x->stream));
    HIPCHK(hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost));
    return 0;
} MN_GUARD_END(set_err, MN_NOTHING, -1)
