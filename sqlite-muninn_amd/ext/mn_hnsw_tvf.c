/*
 * mn_hnsw_tvf.c — hnsw_search_batch, hnsw_search_exact and hnsw_knn_graph: three ADDITIVE eponymous table-valued functions over a
 * live hnsw_index table (mn_vtab_hnsw.h), each a descriptor plus xFilter and xColumn bodies on the scaffold of mn_tvf.h.
 *
 * hnsw_search_batch — many queries, one launch.  The reference's SQL surface answers one query per xFilter
 * (src/hnsw_vtab.c:586-606); this exposes the batched device search without touching hnsw_index:
 *   SELECT query_idx, id, distance FROM hnsw_search_batch
 *    WHERE tbl = 'vec' AND queries = :blob AND k = 10 [AND ef_search = 128];
 * `queries` is nq * dimensions little-endian f32; rows come out grouped by query_idx, ascending distance.
 *
 * hnsw_search_exact is the same function over the exact search (mn_hnsw_search_exact_batch: the true k nearest live rows, ties
 * by insertion order, distances with the bits of the table's own metric), with an optional list of rowids to search among in
 * place of ef_search:
 *   SELECT query_idx, id, distance FROM hnsw_search_exact
 *    WHERE tbl = 'vec' AND queries = :blob AND k = 10 [AND allow = :int64_blob];
 * `allow` is n little-endian int64 rowids; rowids the table does not hold are ignored, an empty blob answers nothing.
 *
 * hnsw_knn_graph — the exact k-NN graph of a table's own rows.  The reference's entity-resolution pipeline
 * (src/llama_er.c:207-286) reads every row of an hnsw_index back, asks the graph for its k + 1 nearest rows and keeps the pairs
 * under a distance threshold: one SELECT and one MATCH per row.  This answers that loop in one statement, exactly, without a
 * vector leaving the device (mn_hnsw_knn_graph): for every live row its k nearest OTHER live rows, ties by insertion order,
 * distances with the bits of the table's own metric, only those with distance <= max_distance when one is given:
 *   SELECT src, dst, distance, rank FROM hnsw_knn_graph WHERE tbl = 'vec' AND k = 10 [AND max_distance = 0.3];
 * src and dst are rowids, rank is 0-based; rows come ordered by (src's insertion order, rank) — an edge list graph_leiden,
 * node2vec_train and graph_closeness take as it is.
 */
#include "mn_tvf.h"
#include "mn_vtab_hnsw.h"

#include <math.h>

enum { BC_QIDX = 0, BC_ID, BC_DIST, BC_TBL };           /* columns of the two searches; hidden: tbl, queries, k, ef_search | allow */
enum { KC_SRC = 0, KC_DST, KC_DIST, KC_RANK, KC_TBL };  /* columns of hnsw_knn_graph; hidden: tbl, k, max_distance */
enum { S_IDS = 0, S_DISTS, S_COUNTS, S_AT, S_SRC };     /* result slots */

static const MnTvf exact_tvf;

static int fail(MnTvfCursor *c, char *msg) {
    mn_tvf_vtab(c)->base.zErrMsg = msg;
    return SQLITE_ERROR;
}

/* the index of the table the statement names, or NULL and the statement's error behind the function's name */
static mn_index *index_of(MnTvfCursor *c, sqlite3_value *tbl, int *dim) {
    MnTvfVtab *vt = mn_tvf_vtab(c);
    char *err = 0;
    mn_index *ix = mn_vtab_hnsw_index_of(vt->db, (const char *)sqlite3_value_text(tbl), dim, &err);
    if (!ix)
        fail(c, sqlite3_mprintf("%s: %s", vt->def->name, err));
    sqlite3_free(err);
    return ix;
}

/* The answer lies grouped, [groups][k] with counts[g] places taken (none of a deleted slot's, count -1).  The cursor walks the
 * taken places in order, at[row] = g * k + rank — which is the row's rowid as well: a short group leaves a gap in the numbering,
 * an empty one is stepped over. */
static int walk_groups(MnTvfCursor *c, const int *counts, int groups, int k) {
    long long rows = 0;
    for (int g = 0; g < groups; g++)
        rows += counts[g] > 0 ? counts[g] : 0;
    long long *at = (long long *)mn_tvf_alloc(c, S_AT, rows, sizeof(long long));
    if (!at)
        return SQLITE_NOMEM;
    long long row = 0;
    for (int g = 0; g < groups; g++)
        for (int r = 0; r < counts[g]; r++)
            at[row++] = (long long)g * k + r;
    c->k = k;
    c->n = rows;
    c->eof = rows == 0;
    return SQLITE_OK;
}

static long long place_of(const MnTvfCursor *c) { return ((const long long *)c->buf[S_AT])[c->pos]; }

static int search_filter(MnTvfCursor *c, int idxNum, int argc, sqlite3_value **argv) {
    const MnTvf *def = mn_tvf_vtab(c)->def;
    const char *fn = def->name;
    const int exact = def == &exact_tvf;
    sqlite3_value *a[MN_TVF_MAX_HIDDEN];
    mn_tvf_args(def, idxNum, argc, argv, a);
    if (!a[0] || !a[1] || !a[2])
        return SQLITE_OK;
    const float *q = (const float *)sqlite3_value_blob(a[1]);
    const int qbytes = sqlite3_value_bytes(a[1]);
    const int k = sqlite3_value_int(a[2]);
    const int ef = a[3] && !exact ? sqlite3_value_int(a[3]) : 2 * k;
    int dim = 0;
    mn_index *ix = index_of(c, a[0], &dim);
    if (!ix)
        return SQLITE_ERROR;
    const int row = dim * (int)sizeof(float);
    if (k <= 0 || qbytes <= 0 || qbytes % row != 0)
        return fail(c, sqlite3_mprintf("%s: queries must be a multiple of %d bytes (%d-dim f32), got %d", fn, row, dim, qbytes));
    const int has_allow = exact && a[3] && sqlite3_value_type(a[3]) != SQLITE_NULL;
    const int64_t *allow = has_allow ? (const int64_t *)sqlite3_value_blob(a[3]) : 0;
    const int abytes = has_allow ? sqlite3_value_bytes(a[3]) : 0;
    if (abytes % 8 != 0)
        return fail(c, sqlite3_mprintf("%s: allow must be a multiple of 8 bytes (int64 rowids), got %d", fn, abytes));
    const int nq = qbytes / row;
    int64_t *ids = (int64_t *)mn_tvf_alloc(c, S_IDS, (long long)nq * k, sizeof(int64_t));
    float *dists = (float *)mn_tvf_alloc(c, S_DISTS, (long long)nq * k, sizeof(float));
    int *counts = (int *)mn_tvf_alloc(c, S_COUNTS, nq, sizeof(int));
    if (!ids || !dists || !counts)
        return SQLITE_NOMEM;
    static const int64_t none = 0; /* an empty blob has no address: any non-NULL pointer says "filter, nothing allowed" */
    if ((exact ? mn_hnsw_search_exact_batch(ix, q, nq, k, has_allow ? (abytes ? allow : &none) : 0, abytes / 8, ids, dists, counts)
               : mn_hnsw_search_batch(ix, q, nq, k, ef, ids, dists, counts)) != 0)
        return fail(c, sqlite3_mprintf("%s: %s", fn, mn_last_error()));
    return walk_groups(c, counts, nq, k);
}

static void search_column(const MnTvfCursor *c, sqlite3_context *ctx, int col) {
    const long long at = place_of(c);
    switch (col) {
    case BC_QIDX: sqlite3_result_int(ctx, (int)(at / c->k)); break;
    case BC_ID: sqlite3_result_int64(ctx, ((const int64_t *)c->buf[S_IDS])[at]); break;
    case BC_DIST: sqlite3_result_double(ctx, (double)((const float *)c->buf[S_DISTS])[at]); break;
    default: sqlite3_result_null(ctx); break;
    }
}

static int knn_filter(MnTvfCursor *c, int idxNum, int argc, sqlite3_value **argv) {
    const MnTvf *def = mn_tvf_vtab(c)->def;
    sqlite3_value *a[MN_TVF_MAX_HIDDEN];
    mn_tvf_args(def, idxNum, argc, argv, a);
    if (!a[0] || !a[1])
        return SQLITE_OK;
    const int k = sqlite3_value_int(a[1]);
    const float r = a[2] && sqlite3_value_type(a[2]) != SQLITE_NULL ? (float)sqlite3_value_double(a[2]) : INFINITY;
    mn_index *ix = index_of(c, a[0], 0);
    if (!ix)
        return SQLITE_ERROR;
    const int n = mn_hnsw_slot_count(ix);
    if (n <= 0 || k < 1 || k > 128) /* an empty table answers nothing; a k out of range is the library's error to word */
        return mn_hnsw_knn_graph(ix, k, r, 0, 0, 0) != 0 ? fail(c, sqlite3_mprintf("%s: %s", def->name, mn_last_error())) : SQLITE_OK;
    int64_t *src = (int64_t *)mn_tvf_alloc(c, S_SRC, n, sizeof(int64_t)); /* the rowid of every slot */
    int64_t *ids = (int64_t *)mn_tvf_alloc(c, S_IDS, (long long)n * k, sizeof(int64_t));
    float *dists = (float *)mn_tvf_alloc(c, S_DISTS, (long long)n * k, sizeof(float));
    int *counts = (int *)mn_tvf_alloc(c, S_COUNTS, n, sizeof(int));
    /* levels and deleted flags, not needed (counts say which slots live): they land where the row index is built afterwards */
    int *scratch = (int *)mn_tvf_alloc(c, S_AT, (long long)n * 2, sizeof(int));
    if (!src || !ids || !dists || !counts || !scratch)
        return SQLITE_NOMEM;
    if (mn_hnsw_export_nodes(ix, src, scratch, scratch + n) != 0 || mn_hnsw_knn_graph(ix, k, r, ids, dists, counts) != 0)
        return fail(c, sqlite3_mprintf("%s: %s", def->name, mn_last_error()));
    return walk_groups(c, counts, n, k);
}

static void knn_column(const MnTvfCursor *c, sqlite3_context *ctx, int col) {
    const long long at = place_of(c);
    switch (col) {
    case KC_SRC: sqlite3_result_int64(ctx, ((const int64_t *)c->buf[S_SRC])[at / c->k]); break;
    case KC_DST: sqlite3_result_int64(ctx, ((const int64_t *)c->buf[S_IDS])[at]); break;
    case KC_DIST: sqlite3_result_double(ctx, (double)((const float *)c->buf[S_DISTS])[at]); break;
    case KC_RANK: sqlite3_result_int(ctx, (int)(at % c->k)); break;
    default: sqlite3_result_null(ctx); break;
    }
}

/* all three: argv in column order, idxNum the bitmask of the hidden columns present (MN_TVF_COMPACTED) */
static const MnTvf batch_tvf = {
    .name = "hnsw_search_batch",
    .schema = "CREATE TABLE x(query_idx INTEGER, id INTEGER, distance REAL, tbl TEXT HIDDEN,"
              " queries BLOB HIDDEN, k INTEGER HIDDEN, ef_search INTEGER HIDDEN)",
    .first_hidden = BC_TBL, .n_hidden = 4, .rule = MN_TVF_COMPACTED, .required_mask = 0x7, .cost = 100.0,
    .filter = search_filter, .column = search_column, .rowid = place_of,
};
static const MnTvf exact_tvf = {
    .name = "hnsw_search_exact",
    .schema = "CREATE TABLE x(query_idx INTEGER, id INTEGER, distance REAL, tbl TEXT HIDDEN,"
              " queries BLOB HIDDEN, k INTEGER HIDDEN, allow BLOB HIDDEN)",
    .first_hidden = BC_TBL, .n_hidden = 4, .rule = MN_TVF_COMPACTED, .required_mask = 0x7, .cost = 100.0,
    .filter = search_filter, .column = search_column, .rowid = place_of,
};
static const MnTvf knn_tvf = {
    .name = "hnsw_knn_graph",
    .schema = "CREATE TABLE x(src INTEGER, dst INTEGER, distance REAL, rank INTEGER, tbl TEXT HIDDEN,"
              " k INTEGER HIDDEN, max_distance REAL HIDDEN)",
    .first_hidden = KC_TBL, .n_hidden = 3, .rule = MN_TVF_COMPACTED, .required_mask = 0x3, .cost = 100.0,
    .filter = knn_filter, .column = knn_column, .rowid = place_of,
};

int mn_register_hnsw_tvfs(sqlite3 *db) {
    int rc = mn_tvf_register(db, &batch_tvf);
    if (rc == SQLITE_OK)
        rc = mn_tvf_register(db, &exact_tvf);
    if (rc == SQLITE_OK)
        rc = mn_tvf_register(db, &knn_tvf);
    return rc;
}
