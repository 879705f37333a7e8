/*
 * mn_traverse_tvf.c — graph_bfs over libmuninn_hip.so.
 * Same eponymous table-valued function as the reference (src/graph_tvf.c:759-967 over run_bfs, :230-309): declared schema,
 * xBestIndex handing the hidden-column constraints over in the order SQLite lists them, xFilter mapping them BY POSITION
 * (:876-887 — so `direction='both'` without `max_depth` lands in max_depth, reads as 0 and answers the start row), defaults
 * (max_depth 100, direction 'forward'), the two error strings, rows in queue order with rowid = position.  The SQL ingest is
 * mn_sql_load_graph (text ids → first-seen indices, lists in table-row order, rows with a NULL endpoint skipped); the traversal
 * is mn_graph_bfs.  graph_shortest_path is mn_path_tvf.c's; graph_dfs is not registered.
 *
 * A translation unit of its own: the integrated build (oracle/Makefile) links the reference's graph_tvf.c, which registers
 * its own graph_bfs, next to this repository's other extension sources — nothing of theirs refers to this file.
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
} BfsVtab;

typedef struct {
    sqlite3_vtab_cursor base;
    char **ids; /* node ids, first-seen order (owned) */
    int n_ids;
    char *start; /* the start node's text when it is the only row (owned) */
    int *node, *depth, *parent;
    long long n, pos;
    int eof;
} BfsCursor;

enum { GB_NODE = 0, GB_DEPTH, GB_PARENT, GB_EDGE_TABLE, GB_SRC, GB_DST, GB_START, GB_MAX_DEPTH, GB_DIRECTION };

static void gb_clear(BfsCursor *c) {
    for (int i = 0; i < c->n_ids; i++)
        free(c->ids[i]);
    free(c->ids);
    free(c->start);
    free(c->node);
    free(c->depth);
    free(c->parent);
    c->ids = 0;
    c->start = 0;
    c->node = c->depth = c->parent = 0;
    c->n_ids = 0;
    c->n = c->pos = 0;
    c->eof = 1;
}

static int gb_connect(sqlite3 *db, void *aux, int argc, const char *const *argv, sqlite3_vtab **out, char **err) {
    (void)aux; (void)argc; (void)argv; (void)err;
    int rc = sqlite3_declare_vtab(db, "CREATE TABLE x("
                                      "  node TEXT, depth INTEGER, parent TEXT,"
                                      "  edge_table TEXT HIDDEN, src_col TEXT HIDDEN, dst_col TEXT HIDDEN,"
                                      "  start_node TEXT HIDDEN, max_depth INTEGER HIDDEN, direction TEXT HIDDEN"
                                      ")");
    if (rc != SQLITE_OK)
        return rc;
    BfsVtab *v = (BfsVtab *)sqlite3_malloc((int)sizeof(BfsVtab));
    if (!v)
        return SQLITE_NOMEM;
    memset(v, 0, sizeof(*v));
    v->db = db;
    *out = &v->base;
    return SQLITE_OK;
}

static int gb_disconnect(sqlite3_vtab *v) {
    sqlite3_free(v);
    return SQLITE_OK;
}

/* gtrav_best_index (:822-838): argvIndex counts up in the order SQLite lists the constraints, whatever the column */
static int gb_best_index(sqlite3_vtab *v, sqlite3_index_info *ii) {
    (void)v;
    int arg = 1;
    for (int i = 0; i < ii->nConstraint; i++) {
        if (!ii->aConstraint[i].usable)
            continue;
        int col = ii->aConstraint[i].iColumn;
        if (col >= GB_EDGE_TABLE && col <= GB_DIRECTION && ii->aConstraint[i].op == SQLITE_INDEX_CONSTRAINT_EQ) {
            ii->aConstraintUsage[i].argvIndex = arg++;
            ii->aConstraintUsage[i].omit = 1;
        }
    }
    ii->estimatedCost = 1000.0;
    return SQLITE_OK;
}

static int gb_open(sqlite3_vtab *v, sqlite3_vtab_cursor **out) {
    (void)v;
    BfsCursor *c = (BfsCursor *)calloc(1, sizeof(BfsCursor));
    if (!c)
        return SQLITE_NOMEM;
    c->eof = 1;
    *out = &c->base;
    return SQLITE_OK;
}

static int gb_close(sqlite3_vtab_cursor *cur) {
    gb_clear((BfsCursor *)cur);
    free(cur);
    return SQLITE_OK;
}

/* whether "SELECT a FROM t WHERE b = ?" compiles: what run_bfs prepares for a direction it follows (:250-265) */
static int gb_columns_exist(sqlite3 *db, const char *t, const char *a, const char *b) {
    char *sql = sqlite3_mprintf("SELECT \"%w\" FROM \"%w\" WHERE \"%w\" = ?", a, t, b);
    if (!sql)
        return 0;
    sqlite3_stmt *st = 0;
    int rc = sqlite3_prepare_v2(db, sql, -1, &st, 0);
    sqlite3_free(sql);
    sqlite3_finalize(st);
    return rc == SQLITE_OK;
}

static int gb_start_only(BfsCursor *c, const char *start) {
    size_t len = strlen(start) + 1;
    c->start = (char *)malloc(len);
    if (!c->start)
        return SQLITE_NOMEM;
    memcpy(c->start, start, len);
    c->n = 1;
    c->eof = 0;
    return SQLITE_OK;
}

static int gb_filter(sqlite3_vtab_cursor *cur, int idxNum, const char *idxStr, int argc, sqlite3_value **argv) {
    (void)idxNum; (void)idxStr;
    BfsCursor *c = (BfsCursor *)cur;
    BfsVtab *vt = (BfsVtab *)cur->pVtab;
    static const char *failed = "graph_bfs: traversal failed (check table/column names exist)";
    gb_clear(c);
    const char *edge_table = 0, *src_col = 0, *dst_col = 0, *start = 0, *direction = "forward";
    int max_depth = 100;
    if (argc >= 1) edge_table = (const char *)sqlite3_value_text(argv[0]); /* by position (:876-887) */
    if (argc >= 2) src_col = (const char *)sqlite3_value_text(argv[1]);
    if (argc >= 3) dst_col = (const char *)sqlite3_value_text(argv[2]);
    if (argc >= 4) start = (const char *)sqlite3_value_text(argv[3]);
    if (argc >= 5) max_depth = sqlite3_value_int(argv[4]);
    if (argc >= 6) direction = (const char *)sqlite3_value_text(argv[5]);
    if (!edge_table || !src_col || !dst_col || !start) {
        vt->base.zErrMsg = sqlite3_mprintf("graph_bfs: requires edge_table, src_col, dst_col, start_node parameters");
        return SQLITE_ERROR;
    }
    if (!direction)
        direction = ""; /* a NULL direction follows no list (the reference compares it as a string and faults) */
    /* run_bfs's own checks, in its order: identifiers, the table, then the statement of each direction it follows */
    int ok = ident_ok(edge_table) && ident_ok(src_col) && ident_ok(dst_col);
    if (ok) {
        char *sql = sqlite3_mprintf("SELECT 1 FROM \"%w\" LIMIT 0", edge_table);
        ok = sql && sqlite3_exec(vt->db, sql, 0, 0, 0) == SQLITE_OK;
        sqlite3_free(sql);
    }
    const int go_forward = !strcmp(direction, "forward") || !strcmp(direction, "both");
    const int go_reverse = !strcmp(direction, "reverse") || !strcmp(direction, "both");
    if (ok && go_forward)
        ok = gb_columns_exist(vt->db, edge_table, dst_col, src_col);
    if (ok && go_reverse)
        ok = gb_columns_exist(vt->db, edge_table, src_col, dst_col);
    if (!ok) {
        vt->base.zErrMsg = sqlite3_mprintf("%s", failed);
        return SQLITE_ERROR;
    }
    if (max_depth <= 0 || (!go_forward && !go_reverse)) /* the start node is popped and not expanded (:280-282) */
        return gb_start_only(c, start);
    mn_graph *g = 0;
    char *err = 0;
    int n = 0;
    if (mn_sql_load_graph(vt->db, "graph_bfs", edge_table, src_col, dst_col, 0, direction, 0, 0, 0, &g, &c->ids, &n, &err) !=
        SQLITE_OK) {
        sqlite3_free(err);
        vt->base.zErrMsg = sqlite3_mprintf("%s", failed);
        return SQLITE_ERROR;
    }
    c->n_ids = n;
    int seed = -1;
    for (int i = 0; g && i < n; i++)
        if (!strcmp(c->ids[i], start)) {
            seed = i;
            break;
        }
    if (seed < 0) { /* an empty table, or no row names the start node */
        if (g)
            mn_graph_destroy(g);
        return gb_start_only(c, start);
    }
    const int dir = go_forward && go_reverse ? 0 : go_reverse ? 2 : 1;
    int64_t row_off[2] = {0, 0};
    const int64_t rows = mn_graph_bfs(g, dir, 1, &seed, max_depth, row_off, 0);
    int rc = rows < 0 ? SQLITE_ERROR : SQLITE_OK;
    if (rc == SQLITE_OK) {
        c->node = (int *)malloc((size_t)rows * sizeof(int));
        c->depth = (int *)malloc((size_t)rows * sizeof(int));
        c->parent = (int *)malloc((size_t)rows * sizeof(int));
        if (!c->node || !c->depth || !c->parent) {
            mn_graph_destroy(g);
            return SQLITE_NOMEM;
        }
        rc = mn_graph_bfs_rows(g, c->node, c->depth, c->parent) == 0 ? SQLITE_OK : SQLITE_ERROR;
    }
    if (rc != SQLITE_OK)
        vt->base.zErrMsg = sqlite3_mprintf("graph_bfs: %s", mn_graph_last_error());
    mn_graph_destroy(g);
    if (rc != SQLITE_OK)
        return rc;
    c->n = rows;
    c->eof = rows == 0;
    return SQLITE_OK;
}

static int gb_next(sqlite3_vtab_cursor *cur) {
    BfsCursor *c = (BfsCursor *)cur;
    c->pos++;
    c->eof = c->pos >= c->n;
    return SQLITE_OK;
}
static int gb_eof(sqlite3_vtab_cursor *cur) { return ((BfsCursor *)cur)->eof; }
static int gb_rowid(sqlite3_vtab_cursor *cur, sqlite3_int64 *out) {
    *out = ((BfsCursor *)cur)->pos;
    return SQLITE_OK;
}

static int gb_column(sqlite3_vtab_cursor *cur, sqlite3_context *ctx, int col) {
    BfsCursor *c = (BfsCursor *)cur;
    switch (col) {
    case GB_NODE:
        sqlite3_result_text(ctx, c->start ? c->start : c->ids[c->node[c->pos]], -1, SQLITE_TRANSIENT);
        break;
    case GB_DEPTH:
        sqlite3_result_int(ctx, c->start ? 0 : c->depth[c->pos]);
        break;
    case GB_PARENT:
        if (c->start || c->parent[c->pos] < 0)
            sqlite3_result_null(ctx);
        else
            sqlite3_result_text(ctx, c->ids[c->parent[c->pos]], -1, SQLITE_TRANSIENT);
        break;
    default:
        sqlite3_result_null(ctx);
        break;
    }
    return SQLITE_OK;
}

static sqlite3_module bfs_module = {
    .iVersion = 0, .xCreate = 0, .xConnect = gb_connect, .xBestIndex = gb_best_index, .xDisconnect = gb_disconnect,
    .xDestroy = gb_disconnect, .xOpen = gb_open, .xClose = gb_close, .xFilter = gb_filter, .xNext = gb_next,
    .xEof = gb_eof, .xColumn = gb_column, .xRowid = gb_rowid,
};

int mn_register_traversal_tvfs(sqlite3 *db) { /* the first of graph_register_tvfs (src/graph_tvf.c:1898-1914) */
    return sqlite3_create_module(db, "graph_bfs", &bfs_module, 0);
}
