// mn_index_int.hpp — what the translation units behind the mn_index handle share: mn_index.hip (handle, id table, host
// metadata, link mirror, delete / load / export), mn_index_search.hip (every search driver) and mn_index_insert.hip (every
// insert and build driver).  Host code only: the kernels live in the units the launchers of mn_device.hpp belong to.
#pragma once
#include "../../include/muninn_hip.h"
#include "mn_comm.hpp"
#include "mn_device.hpp"
#include "mn_guard.hpp"
#include "mn_host.hpp"

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

// the thread's mn_last_error string (mn_index.hip)
void set_err(const char *fmt, ...) __attribute__((format(printf, 1, 2)));
#define HIPCHK(expr) MN_HIPCHK(set_err, expr)

// mn_host.hpp's owned device array with the index's way to a size: geometric steps, an optional fill, mn_last_error
template <typename T> struct IndexBuf : DevBuf<T> {
    using DevBuf<T>::p;
    using DevBuf<T>::cap;
    // `want` (> n, optional): a size the caller knows the buffer will reach (a bulk build) — taken exactly, in ONE allocation,
    // instead of the geometric steps and their 1.5x slack
    int reserve(size_t n, bool keep, hipStream_t st, int fill_byte = -1, size_t want = 0) {
        if (n <= cap)
            return 0;
        size_t nc = cap ? cap : 1024;
        while (nc < n)
            nc = nc + nc / 2 + 1024;
        if (want > n)
            nc = want;
        T *np = nullptr;
        HIPCHK(hipMalloc(&np, nc * sizeof(T)));
        if (fill_byte >= 0)
            HIPCHK(hipMemsetAsync(np, fill_byte, nc * sizeof(T), st));
        if (keep && p && cap)
            HIPCHK(hipMemcpyAsync(np, p, cap * sizeof(T), hipMemcpyDeviceToDevice, st));
        if (p) {
            HIPCHK(hipStreamSynchronize(st));
            HIPCHK(hipFree(p));
        }
        p = np;
        cap = nc;
        return 0;
    }
};

// The index's stream and events.  A base of mn_index, so that they outlive every DevBuf member when an index is deleted: the
// device buffers are freed first, then the events go, then the stream.
struct MnStreamEvents {
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr, ev2 = nullptr;
    ~MnStreamEvents() {
        if (ev0) (void)hipEventDestroy(ev0);
        if (ev1) (void)hipEventDestroy(ev1);
        if (ev2) (void)hipEventDestroy(ev2);
        if (stream) (void)hipStreamDestroy(stream);
    }
};

struct mn_index : MnStreamEvents {
    int device = 0;
    mn_build_stats bstats = {0, 0, 0, 0, 0, 0};
    int dim = 0, ld = 0, metric = 0, order = MN_ORDER_SSE, M = 0, M_max0 = 0, efc = 0;
    int W0 = 0, WU = 0; // row strides of links0 / links_up (>= M_max0 / M; grown when a list must exceed M_max)
    double level_mult = 0;
    int64_t entry_id = -1;
    int max_level = -1;
    unsigned rng_state = 42;
    int node_count = 0;
    int n_deleted = 0; // soft-deleted nodes among the slots
    bool last_on_host = false; // `last` already holds the counters of the last search (the few-queries path)
    int64_t slot_hint = 0; // slots a running bulk build will reach (sync_meta sizes the device tables for it at once)
    // host metadata, slot-indexed
    std::vector<int64_t> ids;
    std::vector<signed char> levels;
    std::vector<unsigned char> deleted;
    std::vector<int> up_off;
    int n_slots = 0, n_pool_rows = 0;
    int meta_uploaded = 0; // slots whose metadata is on the device
    // reference-compatible open-addressing table id → slot (src/hnsw_algo.c:38-91)
    std::vector<int> ht;
    int ht_cap = 256;
    // device state
    IndexBuf<float> d_vectors, d_norms;
    IndexBuf<mn_lo_t> d_vec_lo;    // coded shadow of d_vectors (mn_lo_row_words(ld) dwords per row), grown with it (mn_lo_enabled(ld) only; mn_device.hpp MnLoMeta)
    IndexBuf<MnLoMeta> d_lo_meta;
    IndexBuf<int> d_links0, d_links_up, d_up_off;
    IndexBuf<signed char> d_levels;
    IndexBuf<unsigned char> d_deleted, d_dirty;
    IndexBuf<long long> d_ids;
    // host mirror of the link rows (pulled on demand for delete / inspection / load)
    std::vector<int> h_links0, h_links_up;
    bool host_links_valid = true;   // host mirror == device
    bool dev_links_stale = false;   // host mirror modified, device not yet updated
    bool dev_links_all = false;     // ... and the whole table has to go (load, re-stride); otherwise only h_dirty_rows
    std::vector<std::pair<int, int>> h_dirty_rows; // (slot, level) rows of the mirror edited since the last push
    // nodes appended by mn_hnsw_load_node whose vectors wait on the host for one bulk upload
    std::vector<float> load_vecs;
    int load_first = -1;
    // workspaces
    IndexBuf<unsigned> ws_bm0, ws_bmu;
    IndexBuf<uint2> ws_cand, ws_res;
    IndexBuf<float> ws_q, ws_outd;
    IndexBuf<long long> ws_outi;
    IndexBuf<int> ws_outc, ws_qslots, ws_sel, ws_nsel, ws_upidx;
    IndexBuf<int> lk_target, lk_src, lk_counters, lk_count, lk_fill, lk_binoff, lk_touched, lk_bins, lk_newrows;
    IndexBuf<int> lk_rec, lk_rec_all, lk_cls; // divided link step of the jointly built graph: this rank's records, everybody's, class counts
    IndexBuf<unsigned long long> ws_counters;
    IndexBuf<int> ws_state;
    IndexBuf<int> er_slot, er_level, er_nbr;
    IndexBuf<float> er_dist;
    // speculative exact build: read logs of a window's searches, per-row rewrite epochs
    IndexBuf<int> ws_readlog, ws_nread, ws_ncommit, d_stamp0, d_stampU, d_sidx0, d_sidxU, d_saved_rows, d_pre_act, d_pre_cnt, d_pre_row, d_spec_why;
    int spec_epoch = 0;
    std::vector<int> staged; // mn_hnsw_batch_stage: slots added but not yet searched / linked
    IndexBuf<int> d_staged;
    // multi-GPU exchange buffers (mn_hnsw_build_shared / mn_hnsw_search_sharded)
    IndexBuf<int> sh_sel, sh_nsel, sh_gcnt;
    IndexBuf<int> ws_chlog;            // change log of a single exact insert (mn_hnsw_insert_logged)
    bool want_chlog = false;         // the next run_sequential of one node fills it
    std::vector<int> h_chlog;        // its host copy: [0] entries or -1, then MN_CHLOG_INTS ints each
    // slots whose lists a delete edited: the reference leaves those edits un-persisted (src/hnsw_vtab.c:702-706) until a later
    // insert re-persists the node WHOLE, so an insert that touches one cannot be described by a change log
    std::vector<unsigned char> h_stale;
    int n_stale = 0;
    // pinned host block the kernels of a small search read the queries from and write the answers to (one query per call is
    // the SQL surface's shape: five pageable copies and two synchronisations cost more than the search)
    unsigned char *pin = nullptr;
    size_t pin_cap = 0;
    IndexBuf<unsigned long long> sh_ovf; // [world] heap-workspace overflow counts of the last sharded search, all-gathered
    int sh_ovf_pending = 0;             // entries of sh_ovf not yet looked at by the host (0: none)
    IndexBuf<long long> sh_gids;
    IndexBuf<float> sh_gd;
    long long last_spec_searched = 0; // searches the last speculative build ran (≥ nodes inserted)
    bool broken = false; // an insert failed after its kernels had begun to rewrite link rows: nothing can be trusted
    mn_launch_stats last = {0, 0, 0, 0, 0, 0, 0, 0};
    mn_exact_stats last_exact = {0, 0, 0, 0, 0, 0.0f}; // counters of the last mn_hnsw_search_exact_batch[_dev]
};

// ───────────────────────── mn_index.hip ─────────────────────────
int use_device(mn_index *x); // refuses a broken index, selects the index's device
MnDevIndex dev_view(mn_index *x);
int ht_find(const mn_index *x, int64_t id); // slot of an id, or -1
void ht_grow(mn_index *x);
int random_level(mn_index *x);
int host_add_node(mn_index *x, int64_t id, int level, int deleted); // append a node to the host tables; its slot, or -1
int64_t first_table_full(const mn_index *x, int64_t n);
void mark_stale(mn_index *x, int slot); // a logged insert that touches this slot reports -1 until the node is rewritten whole
// what insert_impl needs to take back the nodes it appended when it fails before any link row was rewritten
struct InsertUndo {
    int first, node_count, max_level, n_pool_rows, old_cap = 0, grew_at = -1;
    unsigned rng;
    int64_t entry_id;
    std::vector<int> old_ht; // the table as it stood just before the call's first growth
};
void undo_insert(mn_index *x, InsertUndo &u);
// make device buffers large enough for the host tables and upload metadata of new slots
int sync_meta(mn_index *x);
// upload n vectors (host [n][dim]) into slots [first, first+n), zero padded to ld, and what is derived from them
int upload_vectors(mn_index *x, int first, const float *vecs, int n, bool src_on_device = false);
int pull_links(mn_index *x); // the host mirror of the link rows made current
int push_links(mn_index *x); // ... and the device's copy, after the mirror was edited
// the index's pinned host block (staging of one insert, mailbox of a small search), at least `need` bytes; nullptr on failure
unsigned char *pin_reserve(mn_index *x, size_t need);
// layout of the block during ONE insert (every piece is consumed before the insert's single synchronisation returns)
#define MN_PIN_META 0      /* up_off, level, deleted, id of the new slot */
#define MN_PIN_IN 64       /* slot, entry slot, max level */
#define MN_PIN_OUT 96      /* state back (2 ints), counters (4 u64) */
#define MN_PIN_VEC 256     /* the vector, zero padded to ld */
inline size_t pin_log_off(const mn_index *x) { return (MN_PIN_VEC + (size_t)x->ld * sizeof(float) + 63) & ~(size_t)63; }
inline size_t pin_insert_bytes(const mn_index *x) {
    return pin_log_off(x) + ((size_t)1 + (size_t)MN_CHLOG_CAP * MN_CHLOG_INTS) * sizeof(int);
}

// ───────────────────────── mn_index_search.hip ─────────────────────────
// The per-query workspace of a search (MnSearchArgs): entries of the candidate and result heaps' spill areas, words of the layer-0
// visited bitmap, and the bytes of the three together.  Words of one upper-layer bitmap (the inserts' searches).
inline int cand_gcap(int ef) { return 16 * ef + 1024; }
inline int res_gcap(int ef) { return ef > MN_RES_LDS ? ef : 8; }
inline int64_t bm0_words(int n_slots) { return ((int64_t)n_slots + 31) / 32; }
inline size_t search_ws_bytes_per_query(int n_slots, int ef) {
    return (size_t)bm0_words(n_slots) * sizeof(unsigned) + ((size_t)cand_gcap(ef) + (size_t)res_gcap(ef)) * sizeof(uint2);
}
inline int64_t bmu_words(const mn_index *x) { return ((int64_t)std::max(1, x->n_pool_rows) + 31) / 32; }
// workspace of a launch over nq queries reserved, zeroed and entered into `a`, with the launch's knobs
int prepare_search_ws(mn_index *x, int64_t nq, int ef, MnSearchArgs &a, bool zero_counters = true, bool lds_bitmap_ok = false);
// x->last from the eight counters of MnSearchArgs::counters ([4] [5] zero: every exact row walked by 4 lanes, as the few-queries
// and insert kernels do); timed: the device time between ev0 and ev1, else 0
void last_from_counters(mn_index *x, const unsigned long long *c, bool timed);
int fetch_counters(mn_index *x); // the same from the device's counters: synchronises
