/*
 * mn_path_tvf.c — graph_shortest_path over libmuninn_hip.so.
 * Same eponymous table-valued function as the reference (src/graph_tvf.c:989-1164 over run_shortest_path_bfs, :472-586, and
 * run_shortest_path_dijkstra, :600-753): declared schema (node, distance, path_order + six hidden columns), xBestIndex handing
 * the hidden-column constraints over in the order SQLite lists them, xFilter mapping them BY POSITION (:1092-1103 — so five
 * constraints whose fifth is weight_col put the weight column's name into end_node), a NULL sixth argument meaning
 * unweighted, the two error strings, rowid = position.  The SQL ingest is mn_sql_load_graph (text ids → first-seen indices,
 * forward lists in table-row order, the weight column read with sqlite3_column_double as the reference reads it); the search
 * is mn_graph_shortest_paths.  MUNINN_GRAPH_MODE = exact → the reference's procedure replayed (its rows), fast → the
 * label-correcting search (its distances, the canonical path), anything else → the library's choice.
 *
 * A translation unit of its own: the integrated build (oracle/Makefile) links the reference's graph_tvf.c, which registers
 * its own graph_shortest_path, next to this repository's other extension sources — nothing of theirs refers to this file.
 */
#include "../../include/muninn_hip.h"
#include "mn_sqlite_abi.h"

#include "mn_nodemap.h"

int mn_sql_load_graph(sqlite3 *db, const char *who, const char *edge_table, const char *src_col, const char *dst_col,
                      const char *weight_col, const char *direction, const char *ts_col, sqlite3_value *t0, sqlite3_value *t1,
                      mn_graph **g_out, char ***ids_out, int *n_out, char **err); /* mn_graph_sql.c */

typedef struct {
    sqlite3_vtab base;
    sqlite3 *db;
} SpVtab;

typedef struct {
    sqlite3_vtab_cursor base;
    char **ids; /* node ids, first-seen order (owned) */
    int n_ids;
    char *start; /* start == end: the one row's text (owned) */
    int *node;
    double *dist;
    long long n, pos;
    int eof;
} SpCursor;

enum { GSP_NODE = 0, GSP_DISTANCE, GSP_PATH_ORDER, GSP_EDGE_TABLE, GSP_SRC, GSP_DST, GSP_START, GSP_END, GSP_WEIGHT };

static void gsp_clear(SpCursor *c) {
    for (int i = 0; i < c->n_ids; i++)
        free(c->ids[i]);
    free(c->ids);
    free(c->start);
    free(c->node);
    free(c->dist);
    c->ids = 0;
    c->start = 0;
    c->node = 0;
    c->dist = 0;
    c->n_ids = 0;
    c->n = c->pos = 0;
    c->eof = 1;
}

static int gsp_connect(sqlite3 *db, void *aux, int argc, const char *const *argv, sqlite3_vtab **out, char **err) {
    (void)aux; (void)argc; (void)argv; (void)err;
    int rc = sqlite3_declare_vtab(db, "CREATE TABLE x("
                                      "  node TEXT, distance REAL, path_order INTEGER,"
                                      "  edge_table TEXT HIDDEN, src_col TEXT HIDDEN, dst_col TEXT HIDDEN,"
                                      "  start_node TEXT HIDDEN, end_node TEXT HIDDEN, weight_col TEXT HIDDEN"
                                      ")");
    if (rc != SQLITE_OK)
        return rc;
    SpVtab *v = (SpVtab *)sqlite3_malloc((int)sizeof(SpVtab));
    if (!v)
        return SQLITE_NOMEM;
    memset(v, 0, sizeof(*v));
    v->db = db;
    *out = &v->base;
    return SQLITE_OK;
}

static int gsp_disconnect(sqlite3_vtab *v) {
    sqlite3_free(v);
    return SQLITE_OK;
}

/* gsp_best_index (:1044-1059): argvIndex counts up in the order SQLite lists the constraints, whatever the column */
static int gsp_best_index(sqlite3_vtab *v, sqlite3_index_info *ii) {
    (void)v;
    int arg = 1;
    for (int i = 0; i < ii->nConstraint; i++) {
        if (!ii->aConstraint[i].usable)
            continue;
        int col = ii->aConstraint[i].iColumn;
        if (col >= GSP_EDGE_TABLE && col <= GSP_WEIGHT && ii->aConstraint[i].op == SQLITE_INDEX_CONSTRAINT_EQ) {
            ii->aConstraintUsage[i].argvIndex = arg++;
            ii->aConstraintUsage[i].omit = 1;
        }
    }
    ii->estimatedCost = 1000.0;
    return SQLITE_OK;
}

static int gsp_open(sqlite3_vtab *v, sqlite3_vtab_cursor **out) {
    (void)v;
    SpCursor *c = (SpCursor *)calloc(1, sizeof(SpCursor));
    if (!c)
        return SQLITE_NOMEM;
    c->eof = 1;
    *out = &c->base;
    return SQLITE_OK;
}

static int gsp_close(sqlite3_vtab_cursor *cur) {
    gsp_clear((SpCursor *)cur);
    free(cur);
    return SQLITE_OK;
}

/* the statement either search prepares before it looks at anything (:478-483, :608-614) */
static int gsp_statement_compiles(sqlite3 *db, const char *t, const char *src, const char *dst, const char *w) {
    char *sql = w ? sqlite3_mprintf("SELECT \"%w\", \"%w\" FROM \"%w\" WHERE \"%w\" = ?", dst, w, t, src)
                  : sqlite3_mprintf("SELECT \"%w\" FROM \"%w\" WHERE \"%w\" = ?", dst, t, src);
    if (!sql)
        return 0;
    sqlite3_stmt *st = 0;
    int rc = sqlite3_prepare_v2(db, sql, -1, &st, 0);
    sqlite3_free(sql);
    sqlite3_finalize(st);
    return rc == SQLITE_OK;
}

/* whether a row of the table (one mn_sql_load_graph would keep: both endpoints present) names `start`, and one `end` */
static int gsp_named(sqlite3 *db, const char *t, const char *src, const char *dst, const char *start, const char *end) {
    char *sql = sqlite3_mprintf("SELECT \"%w\", \"%w\" FROM \"%w\"", src, dst, t);
    sqlite3_stmt *st = 0;
    int has_s = 0, has_e = 0;
    if (sql && sqlite3_prepare_v2(db, sql, -1, &st, 0) == SQLITE_OK)
        while (!(has_s && has_e) && sqlite3_step(st) == SQLITE_ROW) {
            const char *a = (const char *)sqlite3_column_text(st, 0), *b = (const char *)sqlite3_column_text(st, 1);
            if (!a || !b)
                continue;
            has_s |= !strcmp(a, start) || !strcmp(b, start);
            has_e |= !strcmp(a, end) || !strcmp(b, end);
        }
    sqlite3_free(sql);
    sqlite3_finalize(st);
    return has_s && has_e;
}

static int gsp_mode(void) {
    const char *e = getenv("MUNINN_GRAPH_MODE");
    if (e && !strcmp(e, "exact"))
        return MN_SP_REPLAY;
    if (e && !strcmp(e, "fast"))
        return MN_SP_FAST;
    return MN_SP_AUTO;
}

static int gsp_filter(sqlite3_vtab_cursor *cur, int idxNum, const char *idxStr, int argc, sqlite3_value **argv) {
    (void)idxNum; (void)idxStr;
    SpCursor *c = (SpCursor *)cur;
    SpVtab *vt = (SpVtab *)cur->pVtab;
    static const char *failed = "graph_shortest_path: search failed";
    gsp_clear(c);
    const char *edge_table = 0, *src_col = 0, *dst_col = 0, *start = 0, *end = 0, *weight_col = 0;
    if (argc >= 1) edge_table = (const char *)sqlite3_value_text(argv[0]); /* by position (:1092-1103) */
    if (argc >= 2) src_col = (const char *)sqlite3_value_text(argv[1]);
    if (argc >= 3) dst_col = (const char *)sqlite3_value_text(argv[2]);
    if (argc >= 4) start = (const char *)sqlite3_value_text(argv[3]);
    if (argc >= 5) end = (const char *)sqlite3_value_text(argv[4]);
    if (argc >= 6 && sqlite3_value_type(argv[5]) != SQLITE_NULL)
        weight_col = (const char *)sqlite3_value_text(argv[5]);
    if (!edge_table || !src_col || !dst_col || !start || !end) {
        vt->base.zErrMsg = sqlite3_mprintf("graph_shortest_path: requires edge_table, src_col, dst_col, start_node, end_node");
        return SQLITE_ERROR;
    }
    /* both searches: identifiers first, then their statement (:474-483, :603-614) */
    if (!ident_ok(edge_table) || !ident_ok(src_col) || !ident_ok(dst_col) || (weight_col && !ident_ok(weight_col)) ||
        !gsp_statement_compiles(vt->db, edge_table, src_col, dst_col, weight_col)) {
        vt->base.zErrMsg = sqlite3_mprintf("%s", failed);
        return SQLITE_ERROR;
    }
    if (!strcmp(start, end)) { /* the seed is popped and is the end, whether or not a row names it (:511, :672) */
        size_t len = strlen(start) + 1;
        c->start = (char *)malloc(len);
        if (!c->start)
            return SQLITE_NOMEM;
        memcpy(c->start, start, len);
        c->n = 1;
        c->eof = 0;
        return SQLITE_OK;
    }
    if (!gsp_named(vt->db, edge_table, src_col, dst_col, start, end)) /* nothing is found, and no device is asked */
        return SQLITE_OK;
    mn_graph *g = 0;
    char *err = 0;
    int n = 0;
    if (mn_sql_load_graph(vt->db, "graph_shortest_path", edge_table, src_col, dst_col, weight_col, "forward", 0, 0, 0, &g, &c->ids, &n,
                          &err) != SQLITE_OK) {
        sqlite3_free(err);
        vt->base.zErrMsg = sqlite3_mprintf("%s", failed);
        return SQLITE_ERROR;
    }
    c->n_ids = n;
    int s = -1, e = -1;
    for (int i = 0; g && i < n && (s < 0 || e < 0); i++) {
        if (s < 0 && !strcmp(c->ids[i], start))
            s = i;
        if (e < 0 && !strcmp(c->ids[i], end))
            e = i;
    }
    if (s < 0 || e < 0) { /* an empty table, or no row names the start or the end: nothing is found */
        if (g)
            mn_graph_destroy(g);
        return SQLITE_OK;
    }
    int64_t row_off[2] = {0, 0};
    const int64_t rows = mn_graph_shortest_paths(g, gsp_mode(), weight_col != 0, 1, &s, &e, row_off, 0);
    int rc = rows < 0 ? SQLITE_ERROR : SQLITE_OK;
    if (rc == SQLITE_OK && rows > 0) {
        c->node = (int *)malloc((size_t)rows * sizeof(int));
        c->dist = (double *)malloc((size_t)rows * sizeof(double));
        if (!c->node || !c->dist) {
            mn_graph_destroy(g);
            return SQLITE_NOMEM;
        }
        rc = mn_graph_shortest_paths_rows(g, c->node, c->dist) == 0 ? SQLITE_OK : SQLITE_ERROR;
    }
    if (rc != SQLITE_OK)
        vt->base.zErrMsg = sqlite3_mprintf("graph_shortest_path: %s", mn_graph_last_error());
    mn_graph_destroy(g);
    if (rc != SQLITE_OK)
        return rc;
    c->n = rows;
    c->eof = rows == 0;
    return SQLITE_OK;
}

static int gsp_next(sqlite3_vtab_cursor *cur) {
    SpCursor *c = (SpCursor *)cur;
    c->pos++;
    c->eof = c->pos >= c->n;
    return SQLITE_OK;
}
static int gsp_eof(sqlite3_vtab_cursor *cur) { return ((SpCursor *)cur)->eof; }
static int gsp_rowid(sqlite3_vtab_cursor *cur, sqlite3_int64 *out) {
    *out = ((SpCursor *)cur)->pos;
    return SQLITE_OK;
}

static int gsp_column(sqlite3_vtab_cursor *cur, sqlite3_context *ctx, int col) {
    SpCursor *c = (SpCursor *)cur;
    switch (col) {
    case GSP_NODE:
        sqlite3_result_text(ctx, c->start ? c->start : c->ids[c->node[c->pos]], -1, SQLITE_TRANSIENT);
        break;
    case GSP_DISTANCE:
        sqlite3_result_double(ctx, c->start ? 0.0 : c->dist[c->pos]);
        break;
    case GSP_PATH_ORDER:
        sqlite3_result_int(ctx, (int)c->pos);
        break;
    default:
        sqlite3_result_null(ctx);
        break;
    }
    return SQLITE_OK;
}

static sqlite3_module sp_module = {
    .iVersion = 0, .xCreate = 0, .xConnect = gsp_connect, .xBestIndex = gsp_best_index, .xDisconnect = gsp_disconnect,
    .xDestroy = gsp_disconnect, .xOpen = gsp_open, .xClose = gsp_close, .xFilter = gsp_filter, .xNext = gsp_next,
    .xEof = gsp_eof, .xColumn = gsp_column, .xRowid = gsp_rowid,
};

int mn_register_path_tvf(sqlite3 *db) { /* the third of graph_register_tvfs (src/graph_tvf.c:1898-1914) */
    return sqlite3_create_module(db, "graph_shortest_path", &sp_module, 0);
}
