/*
 * muninn_hip.h — C-ABI of libmuninn_hip.so, the MI355X (gfx950) implementation of sqlite-muninn's
 * compute hot path.  Plain pointers and sizes only; no C++/torch types cross this boundary.
 *
 * Each entry point names the reference interface it replaces (file:line in the reference repo).
 * The SQLite glue (hnsw_vtab.c, node2vec.c, graph_community.c) binds to these instead of to
 * hnsw_algo.c / vec_math.c; INTEGRATION.md shows the binding.
 *
 * Threading contract (as the reference's, SURVEY §8b "Threading"): one host thread per index at a
 * time; several indexes per process are fine (each owns a HIP stream).
 *
 * Error convention follows src/hnsw_algo.h:55-79: create → NULL on failure; insert/delete → 0 / -1;
 * search → result count.  mn_last_error() returns a thread-local message for the last failure.
 * There is NO CPU fallback: if no gfx950 device is usable every compute entry point fails.
 */
#ifndef MUNINN_HIP_H
#define MUNINN_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MN_ABI_VERSION 2

/* src/vec_math.h:13 — values are persisted in "{table}_config" (src/hnsw_vtab.c:189) */
typedef enum { MN_METRIC_L2 = 0, MN_METRIC_COSINE = 1, MN_METRIC_INNER_PRODUCT = 2 } mn_metric;

/* Summation order of the distance inner loop:
 *   MN_ORDER_SSE  — bit-exact to the reference's x86 build (src/vec_math.c:78-143)
 *   MN_ORDER_WAVE — wavefront-native order (coalesced float4 per lane + xor butterfly); within
 *                   ~1e-7 relative of the reference, faster */
typedef enum { MN_ORDER_SSE = 0, MN_ORDER_WAVE = 1 } mn_order;

/* Build schedule for mn_hnsw_insert_batch */
typedef enum {
    MN_BUILD_SEQUENTIAL = 0, /* one node at a time: graph bit-identical to hnsw_insert called in a loop */
    MN_BUILD_BATCHED = 1     /* batch-synchronous: nodes of one call are searched against the graph frozen
                                at call start, then linked in order */
} mn_build_mode;

/* src/hnsw_algo.h:30-33 */
typedef struct {
    int64_t id;
    float distance;
} mn_search_result;

typedef struct mn_index mn_index; /* replaces HnswIndex (src/hnsw_algo.h:36-53); device-resident */

/* ---- library ---- */
int mn_abi_version(void);
const char *mn_last_error(void);
/* number of usable gfx950 devices (0 → every compute call fails) */
int mn_device_count(void);
/* Error convention under memory pressure (src/hnsw_algo.h:55-79: hnsw_create → NULL, hnsw_insert / hnsw_delete → -1,
 * hnsw_search → 0): no C++ exception ever leaves this library.  Every entry point that can allocate is closed by an exception
 * barrier (csrc/mn_guard.hpp) which maps std::bad_alloc and friends to the function's error value and names the failure in the
 * thread's last-error string; a call that may have left its handle half-edited marks the handle unusable, later calls on it
 * fail cleanly.  Test hook: the nth host allocation this library makes from now on throws std::bad_alloc (0 disarms);
 * returns the number of host allocations counted since the previous call. */
long long mn_debug_fault_alloc(long long nth);

/* ---- vec_math.c replacements (a1-a4) ---- */
/* src/vec_math.c:192-204: "l2" | "cosine" | "inner_product" → 0, else -1 */
int mn_vec_parse_metric(const char *name, int *out_metric);
/* vec_get_distance_func(metric)(query, rows[i], dim) for i < n  (src/vec_math.c:78-143,180-190).
 * Host pointers; rows is [n][dim] row-major.  Returns 0 / -1 (also when the query and a row, 8 * round_up(dim, 4) bytes, do not
 * fit the LDS the device grants one workgroup: nothing is computed then). */
int mn_vec_dist_batch(int metric, int order, const float *query, const float *rows, int64_t n, int dim, float *out);

/* ---- hnsw_algo.c replacements (a5-a12) ---- */
/* hnsw_create (src/hnsw_algo.c:181-208).  M_max0 = 2M, rng seed 42.  device = HIP ordinal.
 * 2 <= M <= 512 (the reference has no upper bound; here a list of 2M + 1 entries is pruned inside one workgroup's LDS;
 * rows of more than 64 links are walked 64 at a time) and dim <= mn_hnsw_max_dim(M, device) (the reference has no bound either;
 * here kernels stage rows in LDS); NULL + mn_last_error() otherwise, or when no gfx950 device is
 * available (there is no CPU fallback).  The first index a process creates on a device also has HIP load the library's kernels
 * there (tens of milliseconds, once), so that no later query or insert pays for it. */
mn_index *mn_hnsw_create(int dim, int metric, int M, int ef_construction);
mn_index *mn_hnsw_create_on(int dim, int metric, int M, int ef_construction, int device);
/* The largest dim mn_hnsw_create_on accepts for this M on this device: every kernel an index launches must hold its rows in
 * LDS (64 KB, or the device's opt-in limit where a kernel asks for it).  -1 on bad parameters. */
int mn_hnsw_max_dim(int M, int device);
/* hnsw_destroy (:210-220) */
void mn_hnsw_destroy(mn_index *idx);
/* hnsw_seed_rng (:222-224) */
void mn_hnsw_seed_rng(mn_index *idx, unsigned seed);
/* distance summation order for this index; must be set before the first insert (default SSE) */
int mn_hnsw_set_order(mn_index *idx, int order);

/* hnsw_insert (:520-666): vector is copied.  0, or -1 on duplicate id / failure — including the reference's "table full"
 * failure (:61-74): its node table grows on the LIVE count while soft-deleted nodes keep their entries, so delete + insert
 * churn can fill it; as there, the level draw is consumed and nothing else changes. */
int mn_hnsw_insert(mn_index *idx, int64_t id, const float *vector);
/* n inserts in one call.  mode MN_BUILD_SEQUENTIAL ≡ n × mn_hnsw_insert; MN_BUILD_BATCHED is the
 * batch-synchronous schedule.  vectors is host [n][dim].  Returns 0 / -1 (nothing inserted on -1). */
int mn_hnsw_insert_batch(mn_index *idx, const int64_t *ids, const float *vectors, int64_t n, int mode);
/* hnsw_insert that also reports which edges it added / removed, for a host that persists the graph edge by edge (the "{t}_edges"
 * shadow table: src/hnsw_vtab.c:755-776 rewrites every edge of the new node AND of each of its neighbours per insert; with the
 * log only the changed rows are touched).  *n_log = entries written, or -1 when the log cannot describe this insert: more
 * than cap changes, a list wider than 64 links, or a touched node whose persisted copy is not known to match the index —
 * its lists were edited by mn_hnsw_delete (which the reference never persists, src/hnsw_vtab.c:702-706) or the caller said
 * so with mn_hnsw_log_invalidate.  mn_hnsw_take_dirty is then still complete (and taking a node through it makes the node
 * known again); with a valid log the persist set is emptied.  Same graph and return convention as mn_hnsw_insert. */
typedef struct {
    int op;          /* 1: edge src -> dst added at `level` with `distance`;  2: edge src -> dst removed */
    int level;
    int64_t src, dst;
    float distance;  /* dist_func(src vector, dst vector), as persist_node stores it (src/hnsw_vtab.c:262-280) */
} mn_edge_change;
int mn_hnsw_insert_logged(mn_index *idx, int64_t id, const float *vector, mn_edge_change *log, int cap, int *n_log);
/* the caller's persisted copy of these n nodes — or, ids == NULL, of every node present now (a ROLLBACK took rows away that the
 * index keeps) — is not what the index holds: unknown until rewritten whole.  Ids that are not in the index are ignored. */
int mn_hnsw_log_invalidate(mn_index *idx, const int64_t *ids, int64_t n);
/* Bulk build helper: splits [n] into batches growing with the index (batch ≤ max(1, count/grow_div),
 * capped at max_batch) and calls the batched schedule on each.  grow_div ≤ 0 → 16, max_batch ≤ 0 → 8192. */
int mn_hnsw_build(mn_index *idx, const int64_t *ids, const float *vectors, int64_t n, int grow_div, int max_batch);
/* the same from rows already in HBM on the index's device ([n][dim] f32): same batches, same graph; nothing visits the host */
int mn_hnsw_build_dev(mn_index *idx, const int64_t *ids, const float *d_vectors, int64_t n, int grow_div, int max_batch);
int mn_hnsw_device(mn_index *idx); /* HIP ordinal the index lives on */
/* One MN_BUILD_BATCHED batch in three steps, so that several GPUs that each hold a replica of the index can share
 * its search half (the dominant cost) and still all end up with the graph a single GPU builds:
 *   stage  — add the batch's nodes (ids, levels from the index's own level stream, vectors) on this replica;
 *            returns m = nodes waiting to be searched and linked (n, or n-1 when the first node of an empty index
 *            just became the entry point), -1 on error;
 *   search — search staged nodes [lo, hi) against the graph as it stands and write their selected-neighbour lists
 *            into rows lo..hi of the caller's DEVICE arrays d_sel [m][nlev][row_width] / d_nsel [m][nlev]
 *            (mn_hnsw_batch_dims gives nlev = top layer + 1 and row_width = 2M);
 *   (the caller exchanges the rows between replicas — an all-gather — so that every replica holds all m)
 *   link   — apply the whole batch's links from the full arrays and update entry point / top layer.
 * Every replica must stage the same batches in the same order (the level stream is part of the index state). */
int mn_hnsw_batch_stage(mn_index *idx, const int64_t *ids, const float *vectors, int64_t n);
int mn_hnsw_batch_dims(mn_index *idx, int *nlev, int *row_width);
int mn_hnsw_batch_search(mn_index *idx, int lo, int hi, int *d_sel, int *d_nsel);
int mn_hnsw_batch_link(mn_index *idx, const int *d_sel, const int *d_nsel);

/* hnsw_search (:670-704): ef = max(ef, k); results ascending by distance; returns count ≤ k */
int mn_hnsw_search(mn_index *idx, const float *query, int k, int ef_search, mn_search_result *results);
/* nq independent hnsw_search calls in one launch.  queries host [nq][dim]; out_ids/out_dists host
 * [nq][k] (unused tail: id -1, distance 0); out_counts host [nq].  Returns 0 / -1. */
int mn_hnsw_search_batch(mn_index *idx, const float *queries, int64_t nq, int k, int ef_search, int64_t *out_ids,
                         float *out_dists, int *out_counts);
/* Same with every buffer already resident in device memory (HBM) on idx's device; asynchronous on the
 * index's stream — call mn_hnsw_sync before reading.  */
int mn_hnsw_search_batch_dev(mn_index *idx, const float *d_queries, int64_t nq, int k, int ef_search,
                             int64_t *d_out_ids, float *d_out_dists, int *d_out_counts);
int mn_hnsw_sync(mn_index *idx);

/* hnsw_delete (:717-805): soft delete + neighbour reconnection.  0 / -1 (absent or already deleted).  Reconnection may
 * leave a list longer than M_max — the reference's node_add_neighbor grows lists without bound (:142-163) — which the
 * device rows follow (the table is re-strided when a list outgrows the row; the next insert that touches the list prunes it
 * back to M_max exactly as the reference does, :601-646).  Only the few rows of the deleted node's neighbours move
 * between host and device. */
int mn_hnsw_delete(mn_index *idx, int64_t id);

/* hnsw_get_vector / hnsw_get_node (:226-236): copies dim floats out (index lives in HBM).
 * Returns 0, or -1 if absent or deleted. */
int mn_hnsw_get_vector(mn_index *idx, int64_t id, float *out);

/* ---- state the vtab persists / reloads (replaces direct HnswIndex/HnswNode field access in
 *      src/hnsw_vtab.c:237-341,405-462 and ht_find/node_create/node_add_neighbor, src/hnsw_algo.h:98-104) ---- */
int mn_hnsw_node_count(mn_index *idx);     /* live nodes (HnswIndex.node_count) */
int64_t mn_hnsw_entry_point(mn_index *idx); /* -1 if empty */
int mn_hnsw_max_level(mn_index *idx);
int mn_hnsw_node_level(mn_index *idx, int64_t id);   /* -1 if absent */
int mn_hnsw_node_deleted(mn_index *idx, int64_t id); /* -1 if absent */
/* neighbour ids of `id` at `level` in list order; returns the count (may exceed cap), -1 if absent */
int mn_hnsw_neighbors(mn_index *idx, int64_t id, int level, int64_t *out, int cap);
/* load path of load_index_from_shadow (src/hnsw_vtab.c:286-341): nodes first, then edges, then entry.
 * Host-side staging only: vectors and rows reach the device in bulk at the next compute call.
 * mn_hnsw_load_node: 0 = added; 1 = not added because the node table was full or the id is already present — the
 * reference's loop ignores that failure and carries on without the node (:316), and so should the caller; -1 = error.
 * mn_hnsw_load_neighbors: lists may be longer than M_max (a database whose deletes grew them); -1 only on a real error. */
int mn_hnsw_load_node(mn_index *idx, int64_t id, const float *vector, int level, int deleted);
int mn_hnsw_load_neighbors(mn_index *idx, int64_t id, int level, const int64_t *nbrs, int n);
int mn_hnsw_set_entry(mn_index *idx, int64_t entry_point, int max_level);

/* Bulk export (what a bulk persist_node replacement reads, src/hnsw_vtab.c:237-283; also lets a
 * checker mirror the device graph).  Slots are insertion order; deleted nodes keep their slot. */
int mn_hnsw_slot_count(mn_index *idx);
int mn_hnsw_export_nodes(mn_index *idx, int64_t *ids, int *levels, int *deleted); /* each [slot_count] */
int mn_hnsw_export_vectors(mn_index *idx, float *out);                             /* [slot_count][dim] */
/* neighbour rows of every slot at `level` as slot indices, -1 padded: out is [slot_count][width];
 * rows of nodes whose level < `level` are all -1.  *width = mn_hnsw_row_width(idx, level): 2M at level 0, M above,
 * more once a delete or a loaded database has grown a list past that. */
int mn_hnsw_row_width(mn_index *idx, int level);
int mn_hnsw_export_links(mn_index *idx, int level, int *out, int *width);

/* The set of nodes the reference's xUpdate would have re-persisted (src/hnsw_vtab.c:755-768: the new
 * node and every neighbour it linked to), accumulated on the device over all inserts since the last
 * call, so the SQL layer can write shadow tables once per transaction instead of once per row.
 * Fills ids[0..count) in slot order and clears the set; if count > cap nothing is cleared and the
 * count is returned so the caller can retry with room.  -1 on error. */
int64_t mn_hnsw_take_dirty(mn_index *idx, int64_t *ids, int64_t cap);

/* All edges of the given nodes with the distance persist_node stores next to each one
 * (src/hnsw_vtab.c:268-279: dist_func(node, neighbour), 0.0 when the neighbour is soft-deleted).
 * Fills parallel arrays (source id, target id, level, distance) up to `cap`; returns the number of
 * edges (may exceed cap → call again with more room), -1 on error / unknown id. */
int64_t mn_hnsw_edges_of(mn_index *idx, const int64_t *ids, int n, int64_t *out_src, int64_t *out_dst, int *out_level,
                         float *out_dist, int64_t cap);

/* ---- measurement hooks (bench.py) ---- */
typedef struct {
    double last_kernel_ms;   /* HIP-event time of the last dominant kernel launch on the index's stream (0 after a search of a few
                              * host-resident queries, mn_hnsw_search: that path records no events) */
    int64_t last_n_dist;     /* distance evaluations performed by that launch (device counter) */
    int64_t last_n_expanded; /* neighbour rows read by that launch */
    int64_t last_n_overflow; /* queries whose heaps exceeded workspace (must be 0) */
    int64_t last_n_exact_rows; /* f32 rows read for those distances: last_n_dist minus the candidates the coded shadow's bound
                                * rejected (MN_LOWPREC_FILTER; equal to last_n_dist with the filter off) */
    int64_t last_n_rows_lanes4;  /* ... of which walked by 4 lanes per row, */
    int64_t last_n_rows_lanes8;  /* by 8 and */
    int64_t last_n_rows_lanes16; /* by 16 (the filter's survivors in passes with few of them; MN_SURVIVOR_LANES=4|8|16 forces one) */
} mn_launch_stats;
int mn_hnsw_last_launch(mn_index *idx, mn_launch_stats *out);
/* Totals over the batch-synchronous inserts (MN_BUILD_BATCHED / mn_hnsw_build) since the last reset: HIP-event time of
 * the search half (k_beam<BUILD>, the dominant kernel of a build) and of the link half, with the search half's device
 * counters — what the build-side roofline of bench.py is computed from. */
typedef struct {
    double search_ms, link_ms;
    int64_t n_dist, n_expanded; /* distance evaluations / neighbour rows read by the searches */
    int64_t batches, nodes;
} mn_build_stats;
int mn_hnsw_build_stats(mn_index *idx, mn_build_stats *out, int reset);
/* device malloc/free/copies so a non-HIP host (ctypes) can stage HBM-resident inputs */
void *mn_dev_malloc(mn_index *idx, size_t bytes);
void mn_dev_free(mn_index *idx, void *p);
int mn_dev_upload(mn_index *idx, void *dst_dev, const void *src_host, size_t bytes);
int mn_dev_download(mn_index *idx, void *dst_host, const void *src_dev, size_t bytes);
/* exact brute-force top-k on device (ground truth for recall@k; not on the parity path).
 * d_queries device [nq][dim]; out host [nq][k] ids. */
int mn_hnsw_bruteforce_topk(mn_index *idx, const float *d_queries, int64_t nq, int k, int64_t *out_ids);

/* ---- exact (flat) search ----
 * No reference function stands behind these entry points: the reference answers a query only through its graph
 * (hnsw_search, src/hnsw_algo.c:670-704) and computes exact neighbours nowhere but in its benchmark harness, on the CPU.  What
 * they are held to instead is the index's own distance: for every query, d(x) = the value mn_vec_dist_batch returns for the
 * index's metric and order, bit for bit, over all live (non-deleted) slots; the answer is the k smallest under (d ascending as
 * floats, then slot = insertion order ascending), ids and those f32 distances.  1 <= k <= 128.  Output layout of
 * mn_hnsw_search_batch, except that the unused tail of a query with fewer than k live rows is id -1, distance +inf.
 * allow_ids (NULL: no filter): only rows whose id is listed can be returned; unknown and deleted ids are ignored, n_allow = 0
 * with a non-NULL pointer answers nothing.  allow_ids is a HOST array in both calls.
 * The graph and every other piece of index state are left as they were.  DESIGN.md §3.6: a pass on the f32 matrix cores ranks
 * every row by a certified lower bound of d, a short list is re-scored in the index's order, and a per-query certificate
 * proves that no row outside the list could enter the answer; queries it fails for — exact ties at the k-th place among
 * them — and k > 32 run the index's inner loop over every row.  MN_EXACT=valu forces that loop for every query,
 * MN_EXACT_SLACK=<n> sets the list's surplus over k (default 16); both are read per call. */
typedef struct {
    int64_t n_queries, n_mfma_queries, n_fallback_queries, n_rescored_rows, n_bound_violations;
    float kernel_ms;
} mn_exact_stats;
int mn_hnsw_search_exact_batch(mn_index *idx, const float *queries, int64_t nq, int k,
                               const int64_t *allow_ids, int64_t n_allow,   /* allow_ids NULL: no filter */
                               int64_t *out_ids, float *out_dists, int *out_counts);
/* queries and outputs in device memory on idx's device.  Queued on the index's stream, but the call returns only once its
 * kernels have finished: the host reads how many queries failed their certificate before it launches their pass. */
int mn_hnsw_search_exact_batch_dev(mn_index *idx, const float *d_queries, int64_t nq, int k,
                                   const int64_t *allow_ids, int64_t n_allow,
                                   int64_t *d_out_ids, float *d_out_dists, int *d_out_counts);
/* counters of the last exact search on this index: queries asked, queries that took the matrix-core pass, queries whose
 * certificate failed, rows re-scored, and rows whose exact distance lay below their bound (a check of the derivation on every
 * row touched: always 0); kernel_ms = HIP-event time of the call's kernels. */
int mn_hnsw_last_exact(mn_index *idx, mn_exact_stats *out);

/* ---- exact k-NN graph of the index's own rows (the self-join) ----
 * The reference's entity-resolution pipeline (src/llama_er.c:207-286) asks every row of an hnsw_index for its k + 1 nearest rows,
 * one SELECT and one MATCH per row, and keeps the pairs under a distance threshold.  This call gives the exact answer to that loop
 * without a vector leaving the device.  Slots are 0 .. mn_hnsw_slot_count() - 1 in insertion order; a deleted row keeps its slot.
 * For a live slot s the answer is the k smallest rows under (d ascending as floats, slot ascending) among the live slots t != s
 * with d <= max_distance, where d = the bits mn_vec_dist_batch gives for the index's metric and order with row s's stored vector
 * as the query.  The exclusion is by slot: a duplicate of row s is a neighbour like any other.  1 <= k <= 128; max_distance = +inf
 * means no cut, NaN is an argument error.
 * Outputs are indexed by slot: out_ids [slot_count][k] (ids, not slots), out_dists [slot_count][k], out_counts [slot_count];
 * counts[s] = -1 for a deleted slot (its ids -1, distances +inf), else the neighbours kept (0..k); past counts[s]: id -1, +inf.
 * An index without slots answers nothing and returns 0.  The index, its graph and its shadow are left as they were.
 * The slots go through as query batches of MN_KNN_BATCH rows (default 16384, rounded up to a multiple of 128, read per call); each
 * batch takes mn_hnsw_search_exact_batch's passes with the row store as both operands, and MN_EXACT / MN_EXACT_SLACK mean what
 * they mean there.  mn_hnsw_last_exact reports the call summed over its batches: n_queries = the live rows asked. */
int mn_hnsw_knn_graph(mn_index *idx, int k, float max_distance, int64_t *out_ids, float *out_dists, int *out_counts);
/* outputs in device memory on idx's device; returns once the kernels have finished */
int mn_hnsw_knn_graph_dev(mn_index *idx, int k, float max_distance, int64_t *d_out_ids, float *d_out_dists, int *d_out_counts);

/* ---- entity resolution: the middle stages of muninn_extract_er (src/llama_er.c, src/string_sim.c) ----
 * Names are byte strings in one arena: name s is bytes[off[s] .. off[s + 1]), off monotone, no terminator; at most 4096 bytes per
 * name (the reference allocates for any length: a documented deviation, refused before any launch).  Bytes, not code points,
 * as in the reference.  Every argument is checked on the host before anything is launched; errors: -1 + mn_last_error(). */
typedef struct {
    int32_t r1, r2; /* entity indices, r1 < r2 */
    double weight;
} mn_er_edge; /* MatchEdge (src/llama_er.c:41-44) */
typedef enum { MN_ER_GUARD_NONE = 0, MN_ER_GUARD_SAME_SOURCE = 1, MN_ER_GUARD_DIFF_TYPE = 2 } mn_er_guard; /* :130-136 */
typedef enum {
    MN_ER_GRAPH = 0, /* the reference's blocking: every entity's stored vector searched through the graph at k + 1, ef 2 (k + 1) */
    MN_ER_EXACT = 1  /* mn_hnsw_knn_graph at k: the exact neighbours under the threshold */
} mn_er_blocking;
typedef struct {
    int64_t n_candidates, n_edges;
    int64_t n_jw_short, n_jw_long; /* pairs that ran the matching loop one per lane / one per wavefront */
    double blocking_ms, candidates_ms, score_ms; /* device time per stage */
} mn_er_stats;
/* jaro_winkler(name a[p], name b[p]) (src/string_sim.c:11-96) for p < n_pairs, bit-identical f64.  Pairs of names of at most 64
 * bytes go one per lane, longer ones one per wavefront, in the same launch.  0 / -1. */
int mn_er_jaro_winkler(int64_t n_pairs, const unsigned char *bytes, const int64_t *off, int64_t n_str, const int *a, const int *b,
                       int device, double *out);
/* The candidate loop of src/llama_er.c:237-284 over a search's answer: ent_ids[n] are the entities' rowids (unique) in entity order;
 * nbr_ids / nbr_dists [n][kk] and counts[n] each entity's neighbours (count <= 0: the entity has no vector).  An id twice in ent_ids is an
 * argument error (found on the device, reported before any pair is written); an id twice in ONE list — no search answers so — is
 * not checked and leaves the pairs of that id undefined.  An entry survives when its id is not the entity's own, !((double)d > dist_threshold), and the id is an entity.
 * Output: the unordered pairs (r1 < r2, entity indices) in order of first appearance over (entity, list position), each with the
 * smallest distance of its appearances — the reference's list without its linear scan.  r1, r2, dist are the caller's, n * kk
 * entries each.  Returns the pair count, or -1. */
int64_t mn_er_candidates(int n, int kk, const int64_t *ent_ids, const int64_t *nbr_ids, const float *nbr_dists, const int *counts,
                         double dist_threshold, int device, int *r1, int *r2, double *dist);
/* The type guard and scoring cascade of src/llama_er.c:295-332 per candidate, in order: source ids (0 = empty, never blocks; NULL =
 * all empty) against `guard`; names equal -> 1.0; equal after lowering ASCII A-Z -> 0.9; else
 * jw_weight * jaro_winkler(lowered names) + (1.0 - jw_weight) * (1.0 - dist); kept when score >= match_threshold.  edges (the
 * caller's, n_cand entries) receives the kept candidates in candidate order.  Returns the edge count, or -1. */
int64_t mn_er_score(int64_t n_cand, const int *r1, const int *r2, const double *dist, int n, const unsigned char *bytes,
                    const int64_t *off, const int *source_id, int guard, double jw_weight, double match_threshold, int device,
                    mn_er_edge *edges);
/* Stages 2 and 3 of muninn_extract_er (src/llama_er.c:207-332) on the index's device and stream: blocking, candidates, scores.
 * Only names go up and only edges come down.  An entity whose id is absent from the index or deleted has no vector and no list
 * (:240-243).  1 <= k <= 127.  MN_ER_EXACT cuts at the largest float not above dist_threshold, so that the float cut and the
 * reference's double comparison agree on every f32 distance.  edges: the caller's, n * (k + 1) entries.  stats may be NULL.
 * Returns the edge count, or -1. */
int64_t mn_hnsw_er_edges(mn_index *idx, int n, const int64_t *ent_ids, const unsigned char *bytes, const int64_t *off,
                         const int *source_id, int k, double dist_threshold, double jw_weight, double match_threshold, int guard,
                         int blocking, mn_er_edge *edges, mn_er_stats *stats);

/* ---- graph_csr.h / graph_community.c replacements (a18-a22) ---- */
typedef struct mn_graph mn_graph; /* device-resident adjacency: GraphData.out / .in (src/graph_load.h:27-37) as two
                                     CsrArray (src/graph_csr.h:27-34: int32 offsets[V+1], int32 targets[E], f64 weights[E]|NULL) */
/* Per-node edge order must be the adjacency-list order (edge-table row order).  weights NULL = 1.0. */
mn_graph *mn_graph_create(int n_nodes, const int *off_out, const int *tgt_out, const double *w_out, const int *off_in,
                          const int *tgt_in, const double *w_in, int device);
/* The same graph from the reference's stored form: the rows of graph_adjacency's shadow tables
 * "{t}_csr_fwd" / "{t}_csr_rev" (src/graph_adjacency.c:182-197), one mn_csr_block per row in block_id order.  A block
 * holds offsets int32[nodes_in_block + 1] rebased to 0, targets int32[edges] as GLOBAL node indices, weights f64[edges]
 * or nothing (src/graph_csr.c:335-400).  Blocks are uploaded to their place in the device arrays directly — the
 * reference's deserialize → merge → GraphData adjacency-list round trip (src/graph_adjacency.c:1458-1530) has no
 * counterpart.  A single monolithic row (block_size 0) is one block. */
typedef struct {
    const void *offsets;
    int offsets_bytes;
    const void *targets;
    int targets_bytes;
    const void *weights; /* NULL / 0 bytes when unweighted */
    int weights_bytes;
} mn_csr_block;
mn_graph *mn_graph_create_blocked(int n_nodes, const mn_csr_block *fwd, int n_fwd, const mn_csr_block *rev, int n_rev, int device);
/* The same graph from an edge list with integer node indices, built on the device (csrc/mn_csr_build.hip): what the
 * reference's ingest loop (src/graph_load.c:227-246) and csr_build (src/graph_csr.c:20-83) make on the host.  out[src] lists
 * dst and in[dst] lists src, each in edge ROW order; weights (NULL = unweighted) are copied bit for bit.  lists: 1 = out,
 * 2 = in, 3 = both; a list not asked for is empty, as if mn_graph_create had been given empty lists.  The result is an
 * ordinary handle (weighted, edge counts, maximum degrees, host offset copies).  n_rows == 0 is a graph of empty lists.
 * Two implementations give the same bytes: one stable rocprim radix sort of (node, row number) (MN_CSR_BUILD=radix, the
 * default: the faster one on the benchmark graph) and, with MN_CSR_BUILD=sort, per-list sorts of row numbers binned by degree
 * (the bin limits are read per call from MN_CSR_SORT_WAVE, at most 64, and MN_CSR_SORT_LDS, at most 8192).  An index outside 0 .. n_nodes - 1 (found on the device before anything is
 * written through it), n_rows < 0, n_rows >= 2^31 - 1 or n_nodes < 0 is an error: NULL with mn_graph_last_error set.  Sets
 * mn_graph_last_ms (first kernel to last, the offsets' read-back between them included; the uploads are outside). */
mn_graph *mn_graph_from_edges(int n_nodes, int64_t n_rows, const int *src, const int *dst, const double *w, int lists, int device);
/* One direction of the handle as csr_build leaves it on the host (which: 0 = out, 1 = in): off[n_nodes + 1], tgt[edges],
 * w[edges]; tgt and w may be NULL, and w is written only where the graph holds weights for that direction.  Returns 1 when
 * it does, 0 when it does not, -1 on error. */
int mn_graph_export_csr(mn_graph *g, int which, int *off, int *tgt, double *w);
/* A second owner: every mn_graph_retain is paid for by one more mn_graph_destroy, and the last one frees. */
void mn_graph_retain(mn_graph *g);
void mn_graph_destroy(mn_graph *g);
const char *mn_graph_last_error(void);

typedef enum {
    MN_LEIDEN_SEQUENTIAL = 0, /* the reference's in-order sweep with immediate moves: community[] and Q bit-identical */
    MN_LEIDEN_BATCHED = 1     /* parallel schedules: whole-graph synchronous sweeps, or rounds of `batch` nodes */
} mn_leiden_mode;
typedef struct {
    int64_t iterations, moves, move_sweeps, refine_sweeps;
    int n_communities;
    double device_ms;
} mn_leiden_stats;
/* run_leiden (src/graph_community.c:336-429).  use_both = (direction == "both").  community_out[n_nodes] is
 * renumbered 0..K-1 in first-seen order; *modularity_out = Q.  batch (BATCHED only): 0 or 1 → the default schedule, whole-graph
 * synchronous sweeps in which every positive-gain mover applies and every 3rd sweep is "pick-less" (moves to a smaller
 * community id only), finished by the round schedule if 48 sweeps do not settle; < 0 → the same with a pick-less sweep every
 * -batch sweeps; > 1 → rounds of `batch` nodes with the safe-winner commit rule.  Returns 0 / -1. */
int mn_graph_leiden(mn_graph *g, double resolution, int use_both, int mode, int batch, int *community_out,
                    double *modularity_out);
int mn_graph_leiden_stats(mn_graph *g, mn_leiden_stats *out);

/* brandes_compute (src/graph_centrality.c:393-505): node betweenness cb_out[n] and, when eb_out != NULL, the reference's dense
 * edge matrix eb_out[n*n] (EB[v*n + w] = betweenness of v -> w; the reference allocates the same n x n doubles).  BFS for
 * unweighted graphs, Dijkstra for weighted ones; direction 0 = "both" (halved), 1 = "forward", 2 = "reverse";
 * auto_approx > 0 and n > auto_approx → ceil(sqrt(n)) evenly spaced sources, scaled (:420-429); normalized → / ((n-1)(n-2)[/2]).
 * The graph must have been created with the lists the direction traverses (out for 1, in for 2, both for 0), as
 * graph_data_load fills them (src/graph_load.c:144-250).  Bit-identical to the reference.  0 / -1. */
int mn_graph_betweenness(mn_graph *g, int direction, int auto_approx, int normalized, double *cb_out, double *eb_out);
double mn_graph_last_ms(mn_graph *g); /* device time of the last betweenness / closeness call */
/* GraphData.out as CSR on the host (off[n+1], tgt[mn_graph_out_edge_count]) — the order graph_edge_betweenness emits rows in */
long long mn_graph_out_edge_count(mn_graph *g);
int mn_graph_out_lists(mn_graph *g, int *off, int *tgt);

/* clo_filter's per-source loop (src/graph_centrality.c:1396-1434): out[n] = closeness of every node = reachable / sum of
 * distances, times reachable / (n - 1) when normalized.  direction 0 = both, 1 = forward, 2 = reverse, with
 * mn_graph_betweenness's meaning and the same requirement on which lists the graph holds.  Unweighted graphs run a
 * bit-parallel multi-source BFS (64 sources per word: the sum of integer distances is exact in any order), weighted ones
 * the reference's Dijkstra one lane per source.  Sources go through in chunks under a scratch budget: half of the free
 * device memory, or MN_CLOSENESS_SCRATCH_MB MiB (fractions allowed) — 24 bytes per node per batch of 64 sources when
 * unweighted; 12 bytes per node + 16 bytes per (traversed edge + 2) per source when weighted.  n > 2^26 is refused.
 * Bit-identical to the reference; sets mn_graph_last_ms.  0 / -1. */
int mn_graph_closeness(mn_graph *g, int direction, int normalized, double *out);
/* deg_filter's loop (:667-680): sums of out-/in-list weights in list order (1.0 per entry where the graph has no weights; a
 * list the graph does not hold contributes 0), degree = in + out, centrality = degree, or degree / (n - 1) when
 * normalized && n > 1.  Any output pointer may be NULL.  0 / -1. */
int mn_graph_degree(mn_graph *g, int normalized, double *in_deg, double *out_deg, double *degree, double *centrality);

typedef struct {
    int64_t rows, levels, chunks, edges_scanned; /* levels: level passes run, each one host round trip, summed over the chunks */
    double device_ms;
} mn_bfs_stats;
/* run_bfs (src/graph_tvf.c:230-309) for n_seeds start nodes at once: per seed the rows (node, depth, parent) in the order
 * the reference's queue pops them — level by level, a level's nodes ordered by (parent's position in the previous level, index
 * in the parent's list: out-list before in-list, :284-297), the parent being the first neighbour in that order to reach the
 * node; a node at max_depth is not expanded (:282).  A level-synchronous pass over all seeds of a chunk (csrc/mn_bfs.hip): the
 * order is a minimum over edge numbers, so it does not depend on arrival order, launch shape or chunking.  direction 0 = both,
 * 1 = forward, 2 = reverse, with mn_graph_betweenness's meaning and the same requirement on which lists the graph holds (a
 * graph whose lists were filled for another direction is refused).  Seeds may repeat, each gets its own answer; n_seeds == 0
 * answers 0 rows; max_depth <= 0 answers the seed rows; weights are ignored.  row_off[n_seeds + 1]: seed i's rows are
 * row_off[i] .. row_off[i + 1] - 1 of mn_graph_bfs_rows.  Seeds go through in chunks under a scratch budget: half of the free
 * device memory, or MN_BFS_SCRATCH_MB MiB (fractions allowed) — 64 bytes per node per seed of a chunk (4 of them the visited
 * word, filled once per allocation and reset after a chunk only where the chunk's rows name it; the rest bounds the rows and
 * their sort), at least one seed, at most (2^31 - 1) / n; the scratch stays with the handle until mn_graph_destroy.  A seed
 * outside 0 .. n - 1, n_seeds < 0, a missing list, n > 2^26 or more than 2^32 - 3 list entries is an error before any launch.
 * stats may be NULL.  Sets mn_graph_last_ms (the kernels, without the host's waits between levels).  Returns the row count,
 * or -1 with mn_graph_last_error set. */
int64_t mn_graph_bfs(mn_graph *g, int direction, int64_t n_seeds, const int *seeds, int max_depth, int64_t *row_off,
                     mn_bfs_stats *stats);
/* The rows of the last mn_graph_bfs on this handle (they stay with it until the next call or mn_graph_destroy): node, depth and
 * parent (-1 for a seed) of each, row count as returned; any pointer may be NULL.  0 / -1. */
int mn_graph_bfs_rows(mn_graph *g, int *node, int *depth, int *parent);

typedef struct {
    int64_t rows, chunks, entries_scanned, max_frames; /* max_frames: most frames any seed's stack held at once */
    double device_ms;
} mn_dfs_stats;
/* run_dfs (src/graph_tvf.c:322-416) for n_seeds start nodes at once: per seed the rows (node, depth, parent) in the order the
 * reference's stack pops them.  The reference pushes every neighbour that is not visited at that moment (out-list, then
 * in-list, each in table-row order) as an item (node, depth + 1, parent) and drops a popped item whose node is visited, so the
 * last-listed neighbour goes first, a node's depth is that of the item popped first (not its BFS depth), and a node first
 * reached at max_depth is marked, not expanded (:383), and blocks any later, shallower way to it.  The device runs the frame
 * form of the same procedure (csrc/mn_dfs.hip): one frame (u, cursor) per node being expanded, the frame's
 * index its depth, the cursor running from deg(u) down to 0 over out-list ‖ in-list; a step takes the entry below the
 * cursor, and if its node v is not visited marks it, emits (v, depth + 1, u) and, while depth + 1 < max_depth, pushes
 * (v, deg(v)); a frame whose cursor is 0 is popped.  One wavefront per seed reads 64 entries per step.  Conventions of
 * mn_graph_bfs: direction 0 = both, 1 = forward, 2 = reverse and the same requirement on which lists the graph holds; seeds
 * may repeat, each gets its own answer; n_seeds == 0 answers 0 rows; max_depth <= 0 answers the seed rows without a launch;
 * weights are ignored; row_off[n_seeds + 1]: seed i's rows are row_off[i] .. row_off[i + 1] - 1 of mn_graph_dfs_rows, parent
 * -1 for a seed's own row.  Seeds go through in chunks under a scratch budget: half of the free device memory, or
 * MN_DFS_SCRATCH_MB MiB (fractions allowed) — per seed of a chunk 12 bytes per node (its rows) + 4 bytes per 32 nodes (its
 * visited bitmap, cleared per chunk) + 8 bytes per frame, min(n, max_depth) frames; at least one seed; the scratch stays with
 * the handle until mn_graph_destroy.  A seed outside 0 .. n - 1, n_seeds < 0, a missing list, n > 2^26 or 2^31 or more list
 * entries in the lists followed is an error before any launch.  Every seed's step count is bounded on the device by (list
 * entries followed) + 2 n + 2; an overrun is reported as an internal error.  stats may be NULL.  Sets mn_graph_last_ms.
 * Returns the row count, or -1 with mn_graph_last_error set. */
int64_t mn_graph_dfs(mn_graph *g, int direction, int64_t n_seeds, const int *seeds, int max_depth, int64_t *row_off,
                     mn_dfs_stats *stats);
/* The rows of the last mn_graph_dfs on this handle (they stay with it until the next mn_graph_dfs or mn_graph_destroy, and are
 * independent of mn_graph_bfs's): node, depth and parent (-1 for a seed) of each; any pointer may be NULL.  0 / -1. */
int mn_graph_dfs_rows(mn_graph *g, int *node, int *depth, int *parent);

/* ---- graph_shortest_path (src/graph_tvf.c:472-753) ---- */
typedef enum {
    MN_SP_AUTO = 0,      /* replay when the graph holds a negative weight or E_out + 1 <= MN_SP_REPLAY_MAX (4096), else fast */
    MN_SP_REPLAY = 1,    /* run_shortest_path_dijkstra (:600-753) as written, one wavefront per pair: the reference's rows */
    MN_SP_FAST = 2,      /* label-correcting SSSP per distinct start: the reference's distances, canonical parents */
    MN_SP_UNWEIGHTED = 3 /* never asked for, only reported in mn_sp_stats.mode_used: run_shortest_path_bfs (:472-586) */
} mn_sp_mode;
typedef struct {
    int mode_used, chunks, sources; /* sources: distinct starts (fast, unweighted) or pairs (replay) */
    int64_t pops, pushes;           /* replay: queue entries popped (:651-653) and appended (:691-694) */
    int64_t relaxations, passes;    /* fast: list entries relaxed, frontier passes (each one host round trip); unweighted: the
                                       traversals' edges_scanned and levels */
    double device_ms;
} mn_sp_stats;
/* graph_shortest_path's search (src/graph_tvf.c:472-753) for n_pairs (start[i], end[i]) pairs over the handle's out-lists: per
 * pair the rows (node, distance) of one shortest path, start first; no path → no rows; start == end → the one row (start, 0.0).
 * row_off[n_pairs + 1]: pair i's rows are row_off[i] .. row_off[i + 1] - 1 of mn_graph_shortest_paths_rows, and a row's
 * path_order (:730) is its place within the pair.
 *   weighted == 0, or a graph without weights: run_shortest_path_bfs (:472-586), first-discovery parents of one mn_graph_bfs
 *     traversal per distinct start (which replaces the rows of the handle's last mn_graph_bfs); distance = place on the path.
 *   MN_SP_REPLAY: run_shortest_path_dijkstra (:600-753) verbatim — array queue, first index of the strict minimum popped,
 *     last entry into the hole, stale pops dropped, unsettled targets appended in list order — one wavefront per pair.  Every
 *     tie, every finite negative weight and +inf come out as the reference's.  O(pops x queue / 64) per pair.  Scratch per
 *     pair: 16 bytes per (E_out + 1) queue entries and 12 per node.
 *   MN_SP_FAST: weights must be >= 0.  The distances are the reference's bit for bit (with weights >= 0 the fixpoint of
 *     dist[v] = min fl(dist[u] + w) does not depend on the order of relaxations); the path is the canonical one: fewest edges
 *     among the shortest paths, then at each node the parent with the lowest (index, place in its list).  Where only one
 *     shortest path exists that is the reference's.  A start's search ends once all of its ends are final.  Scratch: 40 bytes
 *     per node per distinct start of a chunk.  MN_SSSP_DELTA (a distance, `inf` = plain frontier Bellman-Ford; default: the
 *     mean finite weight) sets the near/far threshold step and changes no output bit, nor does the chunking.
 * Pairs (replay) or distinct starts (fast) go through in chunks under a scratch budget: half of the free device memory, or
 * MN_SP_SCRATCH_MB MiB (fractions allowed), at least one at a time.  A NaN or -inf weight is refused in every weighted mode, a
 * negative weight in MN_SP_FAST; an index outside 0 .. n - 1, n_pairs < 0, a graph that holds only in-lists or n > 2^26 is
 * an error before any launch.  stats may be NULL.  Sets mn_graph_last_ms.  Returns the row count, or -1 with
 * mn_graph_last_error set. */
int64_t mn_graph_shortest_paths(mn_graph *g, int mode, int weighted, int64_t n_pairs, const int *start, const int *end,
                                int64_t *row_off, mn_sp_stats *stats);
/* The rows of the last mn_graph_shortest_paths on this handle (they stay with it until the next call or mn_graph_destroy), the
 * PathRow fields node and distance (:424-428, :729-731); either pointer may be NULL.  0 / -1. */
int mn_graph_shortest_paths_rows(mn_graph *g, int *node, double *distance);

/* ---- graph_select: the lineage selectors (src/graph_selector_parse.c, src/graph_selector_eval.c) ---- */
typedef enum {
    MN_SEL_NODE = 0,        /* x       direction "self" */
    MN_SEL_ANCESTORS = 1,   /* N+x     "ancestor" */
    MN_SEL_DESCENDANTS = 2, /* x+M     "descendant" */
    MN_SEL_BOTH = 3,        /* N+x+M   "both" */
    MN_SEL_CLOSURE = 4,     /* @x      "closure" */
    MN_SEL_UNION = 5,       /* a b     "selected", as the two below */
    MN_SEL_INTERSECT = 6,   /* a,b */
    MN_SEL_COMPLEMENT = 7   /* not a */
} mn_select_opcode;
typedef struct {
    int op;                   /* mn_select_opcode */
    int node;                 /* atoms: the node's index; -1 as parsed, the caller resolves the name */
    int depth_up, depth_down; /* atoms: the limits, -1 = none */
    int name_off, name_len;   /* atoms: where the name stands in the parsed text */
} mn_select_op;
typedef struct {
    int64_t rows, levels, launches, syncs, bottom_up_levels; /* levels: level launches that had a frontier to expand; launches: all
                                                                level launches; syncs: status read-backs, one per group of levels */
    double device_ms;
} mn_select_stats;
/* selector_parse (src/graph_selector_parse.c:467-510) as a postfix program: the atoms stand in source order, a set operator
 * after its operands (union by juxtaposition and intersection by comma are left-associative, `not` binds one atom).  A caller
 * that resolves the atoms' names in program order and stops at the first it does not know reports the node the reference
 * reports.  Same tokens and quirks as the reference: names start with an ASCII letter, digit or '_' and go on with those, '.'
 * and '-'; `not` is a name where the text ends or a comma follows; an all-digit token is a depth only in front of '+'; a '+'
 * after a name is its suffix only if an integer, the end or a comma follows; `@+x` and `@x+` are `@x`.  A depth beyond INT_MAX
 * is INT_MAX (the reference's int overflows there).  *prog is malloc'ed: mn_host_free.  Touches no device.  Returns 0, or -1 with
 * mn_graph_last_error holding the reference's message ("graph_select: empty selector expression", "… unexpected character
 * '%c' at position %d", "… expected node name at position %d", "… unexpected token at position %d"). */
int mn_select_parse(const char *expr, mn_select_op **prog, int *n_ops);
/* selector_eval (src/graph_selector_eval.c:511-543) on the device over the handle's out- and in-lists as they are (the graph must
 * hold both: graph_select loads its table with direction "both").  The rows are the selected nodes in ascending index with
 * their depth: the hop distance the ROOT operator's traversal found (0 for every row when the root is a set operator, and for
 * every descendant under `@x`).  A limit on `N+x` / `x+M` under a set operator is ignored unless it is 0, as in the reference;
 * `N+x+M` honours its limits everywhere, and its descendant pass neither reports nor walks through what its ancestor pass found.
 * A stack machine over n-bit sets (csrc/mn_select.hip): level-synchronous traversals with bitmap frontiers, one launch per level,
 * top-down or bottom-up per level — MN_SELECT_BOTTOM_UP = 0 | 1 | auto (default: bottom-up when the frontier holds more than
 * 1 / MN_SELECT_BOTTOM_UP_DIV of the direction's list entries) — and MN_SELECT_LEVELS_PER_SYNC level launches queued per status
 * read-back; all three are read at each call and change no row.  A node outside 0 .. n - 1, an operator without its operands or
 * a program that does not leave one set is an error before any launch.  The scratch (a few n-bit sets, three int32[n]) stays with the
 * handle until mn_graph_destroy.  stats may be NULL.  Sets mn_graph_last_ms.  Returns the row count, or -1 with
 * mn_graph_last_error set. */
int64_t mn_graph_select(mn_graph *g, const mn_select_op *prog, int n_ops, mn_select_stats *stats);
/* The rows of the last mn_graph_select on this handle: node and depth of each, row count as returned; either may be NULL.  0 / -1. */
int mn_graph_select_rows(mn_graph *g, int *node, int *depth);

/* ---- node2vec.c replacements (a14-a17) ---- */
typedef struct {
    int dim;            /* 1..1024 (src/node2vec.c:447) */
    double p, q;        /* return / in-out parameters */
    int num_walks, walk_length, window, neg_samples;
    double learning_rate;
    int epochs;
    int batch_walks; /* MN_N2V_BATCHED only: walks per batch; <= 0 → clamp(n/64, 1, 16384) */
} mn_n2v_params;
typedef enum {
    MN_N2V_SEQUENTIAL = 0, /* the reference's single serial SGD stream: output bytes identical to the reference's */
    MN_N2V_BATCHED = 1     /* batch-synchronous mini-batch schedule: one wavefront per walk,
                              per-walk RNG streams, deterministic per-row accumulation; bit-identical to the CPU
                              restatement of the same schedule, statistically equivalent to the serial stream */
} mn_n2v_mode;
typedef struct {
    int64_t pairs;    /* (center, context) pairs trained */
    double device_ms;
} mn_n2v_stats;
/* The compute of node2vec_train (src/node2vec.c:486-551): sgns_create (rng 42), walks + SGNS, L2 normalisation.
 * Graph = node2vec.c's own adjacency (first-seen node order, undirected, de-duplicated, :72-138) as CSR:
 * neighbours of node i are adj[off[i] .. off[i+1]) in list order.  out is host [n][dim] f32 — the vectors the
 * reference INSERTs with rowid = i + 1 (:575).  Returns n, or -1. */
int mn_node2vec_train(int n_nodes, const int *off, const int *adj, const mn_n2v_params *prm, int mode, int device, float *out,
                      mn_n2v_stats *stats);
const char *mn_node2vec_last_error(void);
/* node2vec_train's compute AND its output step (src/node2vec.c:540-583: every embedding INSERTed into the output hnsw_index,
 * rowid = first-seen index + 1) without the embeddings leaving HBM: trained (MN_N2V_BATCHED) and normalised on idx's device,
 * then mn_hnsw_build_dev with rowids first_rowid + i.  host_out (or NULL): the embeddings as well, one bulk copy, for a host
 * that persists them.  *build_seconds (or NULL): wall time of the index build.  Same embedding bytes as mn_node2vec_train, same
 * graph as mn_hnsw_build on them.  Returns n, or -1. */
int mn_node2vec_train_into(int n_nodes, const int *off, const int *adj, const mn_n2v_params *prm, int mode, mn_index *idx,
                           int64_t first_rowid, float *host_out, mn_n2v_stats *stats, double *build_seconds);

/* The batched schedule as a session, so that several GPUs can share one training run: every rank produces the
 * samples of its slice of a batch's walks, the (centre, target, err) triples are exchanged (RCCL all-gather, rank
 * order = walk order) and every replica applies the whole batch — the N-GPU embeddings are bit-identical to the
 * 1-GPU ones.  Buffers passed to samples/apply are DEVICE pointers on the session's device; both calls are queued on the
 * session's own stream (in call order) and return at once — mn_n2v_sync before another stream or the host touches the
 * buffers. */
typedef struct mn_n2v_session mn_n2v_session;
mn_n2v_session *mn_n2v_begin(int n_nodes, const int *off, const int *adj, const mn_n2v_params *prm, int device);
int mn_n2v_batch_walks(mn_n2v_session *s);  /* resolved walks per batch */
int mn_n2v_sample_slots(mn_n2v_session *s);   /* sample slots per walk = walk_length * 2*window * (1+neg) */
int mn_n2v_position_slots(mn_n2v_session *s); /* position slots per walk = walk_length */
/* walks of start nodes [lo, hi) (hi - lo <= batch_walks) of pass (epoch, w).  Per walk: `sample_slots` (centre,
 * target, err) triples — the target-side updates, unused slots carry -1 — and `position_slots` (centre, neu1e[dim])
 * entries — the centre-side update of each walk position (src/node2vec.c:347,:383-391), -1 past the walk's end. */
int mn_n2v_samples(mn_n2v_session *s, int epoch, int w, int lo, int hi, int *d_center, int *d_target, float *d_err,
                   int *d_pos_center, float *d_pos_neu);
/* applies ns sample slots and np position slots in the given order (any concatenation of mn_n2v_samples outputs) */
int mn_n2v_apply(mn_n2v_session *s, const int *d_center, const int *d_target, const float *d_err, int64_t ns,
                 const int *d_pos_center, const float *d_pos_neu, int64_t np);
int mn_n2v_sync(mn_n2v_session *s);
int mn_n2v_finish(mn_n2v_session *s, float *out, mn_n2v_stats *stats); /* L2 normalise, download [n][dim] */
/* L2 normalise and leave the embeddings in HBM: *d_out = [n][dim] f32 on the session's device, valid until mn_n2v_end */
int mn_n2v_finish_dev(mn_n2v_session *s, const float **d_out, mn_n2v_stats *stats);
void mn_n2v_end(mn_n2v_session *s);

/* ---- graph_tvf.c's remaining edge-list algorithms ----
 * Nodes are first-seen indices (src of row 0, dst of row 0, src of row 1, ... as pr_adj_find_or_add / uf_find_or_add
 * number them, src/graph_tvf.c:1591-1613,1231-1247); src[e] -> dst[e] are the edge table's rows in order, duplicates and
 * self loops kept as the reference keeps them.  Host arrays. */
typedef struct {
    double device_ms;
    int iterations; /* PageRank: iterations run; components: hook rounds */
    int64_t aux;    /* PageRank: dangling nodes */
} mn_graph_algo_stats;
/* run_pagerank (src/graph_tvf.c:1631-1797): rank_out[n] f64, bit-identical to the reference's sequential push loop
 * (the same additions in the same order, pulled per target).  0 / -1. */
int mn_graph_pagerank(int n_nodes, int64_t n_edges, const int *src, const int *dst, double damping, int iterations, int device,
                      double *rank_out, mn_graph_algo_stats *stats);
typedef enum {
    MN_COMPONENTS_EXACT = 0, /* the reference's union sequence replayed: component_id = its union-find root */
    MN_COMPONENTS_FAST = 1   /* parallel hooking: same partition and sizes, component_id = smallest node index */
} mn_components_mode;
/* run_components (src/graph_tvf.c:1314-1366): component_id[n], component_size[n].  0 / -1. */
int mn_graph_components(int n_nodes, int64_t n_edges, const int *src, const int *dst, int mode, int device, int *component_id,
                        int *component_size, mn_graph_algo_stats *stats);
const char *mn_graph_algo_last_error(void);

/* csr_apply_delta (src/graph_csr.c:175-325), the merge step of graph_adjacency's incremental rebuild
 * (src/graph_adjacency.c:721-1005): old CSR + delta log -> new CSR; per node the log is replayed in order (INSERT appends,
 * DELETE removes the first occurrence by moving the last element into its place), so lists come out in the reference's
 * order.  Host arrays in; new_offsets[max(new_node_count, old_node_count) + 1] is the caller's, *new_targets /
 * *new_weights are malloc'ed here (NULL when the result has no edges; release with mn_host_free).  mn_csr_delta has the
 * layout of CsrDelta (src/graph_csr.h:37-42).  0 / -1. */
typedef struct {
    int32_t src_idx, dst_idx;
    double weight;
    int op; /* 1 = INSERT, 2 = DELETE */
} mn_csr_delta;
int mn_csr_apply_delta(int old_node_count, const int *old_offsets, const int *old_targets, const double *old_weights,
                       int has_weights, const mn_csr_delta *deltas, int delta_count, int new_node_count, int device,
                       int *new_offsets, int **new_targets, double **new_weights, int *new_edge_count);
void mn_host_free(void *p);

/* ---- multi-GPU: one rank per GPU of a node, processes or threads; RCCL over xGMI ----
 * The reference is single-device; these entry points are what its host (hnsw_vtab.c / node2vec.c) would call to use the
 * node's other GPUs.  The only collective is an all-gather of equal-sized device buffers:
 *   RCCL transport: rank 0 calls mn_comm_unique_id and hands the 128 bytes to the other ranks by whatever means the
 *     host has (a file, a socket, MPI, torch.distributed's store); every rank then calls mn_comm_init_rccl.  librccl is
 *     loaded on first use, so single-GPU users never touch it.
 *   host transport: the caller provides the all-gather over HOST buffers (recv = world x bytes_per_rank, rank order) —
 *     rehearsals where several ranks share one GPU (RCCL refuses that), or a host with its own fabric. */
typedef struct mn_comm mn_comm;
#define MN_COMM_ID_BYTES 128
typedef int (*mn_host_allgather_fn)(void *user, const void *send, void *recv, size_t bytes_per_rank);
int mn_comm_unique_id(void *id128);
mn_comm *mn_comm_init_rccl(int world, int rank, const void *id128, int device);
mn_comm *mn_comm_init_host(int world, int rank, mn_host_allgather_fn fn, void *user, int device);
int mn_comm_world(mn_comm *c);
int mn_comm_rank(mn_comm *c);
void mn_comm_destroy(mn_comm *c);
const char *mn_comm_last_error(void);

/* mn_hnsw_build on `world` GPUs that each hold a replica of ONE index: the batches are those of mn_hnsw_build; inside a
 * batch rank r searches a contiguous slice of the batch's nodes against its replica (k_beam<BUILD>, the dominant cost),
 * the selected-neighbour lists are all-gathered and every replica links the whole batch.  Every replica ends with the
 * graph a single GPU builds, bit for bit.  ids / vectors: the SAME host arrays on every rank.  Batches below min_split
 * nodes (<= 0 -> 256) are searched whole by every rank (no exchange).  0 / -1. */
int mn_hnsw_build_shared(mn_index *idx, mn_comm *c, const int64_t *ids, const float *vectors, int64_t n, int grow_div,
                         int max_batch, int min_split);
/* BASELINE config 3: the index is sharded (rowid mod world -> one HNSW graph per GPU, built independently); every rank
 * searches the SAME queries on its shard, the per-shard top-k — k x (int64 id, f32 distance) per query — are all-gathered
 * and merged on the device in the total order (distance, shard rank, position).  Every rank receives the merged result.
 * Device buffers on idx's device; asynchronous on the index's stream like mn_hnsw_search_batch_dev. */
int mn_hnsw_search_sharded_dev(mn_index *idx, mn_comm *c, const float *d_queries, int64_t nq, int k, int ef_search,
                               int64_t *d_out_ids, float *d_out_dists, int *d_out_counts);
/* the same with host buffers */
int mn_hnsw_search_sharded(mn_index *idx, mn_comm *c, const float *queries, int64_t nq, int k, int ef_search, int64_t *out_ids,
                           float *out_dists, int *out_counts);
/* MN_N2V_BATCHED data-parallel over the ranks (BASELINE config 4): every rank holds a replica of both matrices and computes
 * the samples of its contiguous slice of each batch's walks.  A sample is then sent to the ONE rank that owns its target row
 * (a position's neu1e to the owner of its centre row): buckets by destination shard, stable, exchanged all-to-all (ncclSend /
 * ncclRecv over xGMI: 1 / world of the bytes an all-gather moves); every rank sorts and applies what it received to its rows
 * — received buckets stand in rank order = walk order, so a row gets the additions, in the order, one GPU gives it — and the
 * updated row shards of both matrices are all-gathered.  The embeddings are bit-identical to mn_node2vec_train(..,
 * MN_N2V_BATCHED) on one GPU.  stats->pairs is this rank's share.  Returns n / -1. */
int mn_node2vec_train_shared(mn_comm *c, int n_nodes, const int *off, const int *adj, const mn_n2v_params *prm, int device,
                             float *out, mn_n2v_stats *stats);
/* run_leiden (src/graph_community.c:336-429) on the ranks' GPUs — north_star: the per-node local-move sweep "partitioned
 * across the GPUs ... modularity partials".  Every rank holds the whole graph (g on its own device) and the whole state; the
 * evaluation of every synchronous sweep is divided by node range, the decisions (N int32 per sweep) are all-gathered and every
 * replica applies all of them; compute_modularity's per-node terms (:131) are divided and all-gathered the same way.  Every
 * rank returns what mn_graph_leiden(g, .., MN_LEIDEN_BATCHED, batch, ..) returns on one GPU, bit for bit.  0 / -1. */
int mn_graph_leiden_shared(mn_graph *g, mn_comm *c, double resolution, int use_both, int batch, int *community_out,
                           double *modularity_out);

/* ---- the same sharded index (BASELINE config 3) inside ONE process: a C host that owns several GPUs ----
 * rowid mod n -> shard; every shard is an ordinary mn_index on its own GPU (mn_shards_index gives access for persistence:
 * mn_hnsw_take_dirty etc.).  A search uploads the queries to every shard's GPU, searches all shards at once (one stream
 * per GPU, queued by the calling thread), copies the per-shard top-k to the first shard's GPU (hipMemcpyPeerAsync) and
 * merges there with the kernel mn_hnsw_search_sharded uses — the same result, bit for bit, as one rank per GPU over RCCL.
 * devices may repeat an ordinal (several shards on one GPU).  What a loadable extension would bind for
 * MUNINN_DEVICE=0,1,...: hnsw_vtab.c's hnsw_insert / hnsw_search / hnsw_delete call sites (src/hnsw_vtab.c:748, :604,
 * :698) take these instead of the single-index calls.  Errors: mn_shards_last_error(). */
typedef struct mn_shards mn_shards;
mn_shards *mn_shards_create(int dim, int metric, int M, int ef_construction, const int *devices, int n);
void mn_shards_destroy(mn_shards *s);
int mn_shards_count(const mn_shards *s);
mn_index *mn_shards_index(mn_shards *s, int i);
int mn_shards_of(const mn_shards *s, int64_t id); /* ((id mod n) + n) mod n */
int mn_shards_set_order(mn_shards *s, int order);
int mn_shards_insert(mn_shards *s, int64_t id, const float *vector);   /* hnsw_insert on the id's shard */
int mn_shards_delete(mn_shards *s, int64_t id);                         /* hnsw_delete on the id's shard */
/* mn_hnsw_build per shard (input order kept inside every shard), the shards built side by side: one host thread per GPU */
int mn_shards_build(mn_shards *s, const int64_t *ids, const float *vectors, int64_t n, int grow_div, int max_batch);
int mn_shards_search(mn_shards *s, const float *query, int k, int ef_search, mn_search_result *results);
int mn_shards_search_batch(mn_shards *s, const float *queries, int64_t nq, int k, int ef_search, int64_t *out_ids,
                           float *out_dists, int *out_counts);
const char *mn_shards_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* MUNINN_HIP_H */
