/*
 * mn_traverse_tvf.c — graph_bfs and graph_dfs over libmuninn_hip.so: two descriptors, one xFilter and one xColumn on the
 * scaffold of mn_tvf.h.  Same eponymous table-valued functions as the reference (src/graph_tvf.c:759-967 over run_bfs, :230-309,
 * and run_dfs, :322-416; which of the two a table is, is the reference's is_dfs, here the descriptor): declared schema,
 * xBestIndex handing the hidden-column constraints over in the order SQLite lists them, xFilter mapping them BY POSITION
 * (:876-887 — so `direction='both'` without `max_depth` lands in max_depth, reads as 0 and answers the start row), defaults
 * (max_depth 100, direction 'forward'), the two error strings under the function's own name (:890-905), rows in the queue's
 * (graph_bfs) or the stack's (graph_dfs) pop order with rowid = position.  The SQL ingest is
 * mn_sql_load_graph (text ids → first-seen indices, lists in table-row order, rows with a NULL endpoint skipped); the traversal
 * is mn_graph_bfs or mn_graph_dfs (§7.9).  graph_shortest_path is mn_path_tvf.c's.
 *
 * A translation unit of its own: the integrated build (oracle/Makefile) links the reference's graph_tvf.c, which registers
 * its own graph_bfs and graph_dfs, next to this repository's other extension sources — nothing of theirs refers to this file.
 */
#include "mn_tvf.h"

#include "mn_nodemap.h"

enum { GB_NODE = 0, GB_DEPTH, GB_PARENT, GB_EDGE_TABLE }; /* columns; the result slots are node, depth, parent */

static const MnTvf dfs_tvf;

/* whether "SELECT a FROM t WHERE b = ?" compiles: what run_bfs and run_dfs prepare for a direction it follows (:250-265) */
static int gb_columns_exist(sqlite3 *db, const char *t, const char *a, const char *b) {
    return mn_sql_compiles(db, "SELECT \"%w\" FROM \"%w\" WHERE \"%w\" = ?", a, t, b);
}

static int gb_filter(MnTvfCursor *c, int idxNum, int argc, sqlite3_value **argv) {
    (void)idxNum;
    MnTvfVtab *vt = mn_tvf_vtab(c);
    const int is_dfs = vt->def == &dfs_tvf;
    const char *const name = vt->def->name;
    const char *edge_table = 0, *src_col = 0, *dst_col = 0, *start = 0, *direction = "forward";
    int max_depth = 100;
    if (argc >= 1) edge_table = (const char *)sqlite3_value_text(argv[0]); /* by position (:876-887) */
    if (argc >= 2) src_col = (const char *)sqlite3_value_text(argv[1]);
    if (argc >= 3) dst_col = (const char *)sqlite3_value_text(argv[2]);
    if (argc >= 4) start = (const char *)sqlite3_value_text(argv[3]);
    if (argc >= 5) max_depth = sqlite3_value_int(argv[4]);
    if (argc >= 6) direction = (const char *)sqlite3_value_text(argv[5]);
    if (!edge_table || !src_col || !dst_col || !start) {
        vt->base.zErrMsg = sqlite3_mprintf("%s: requires edge_table, src_col, dst_col, start_node parameters", name);
        return SQLITE_ERROR;
    }
    if (!direction)
        direction = ""; /* a NULL direction follows no list (the reference compares it as a string and faults) */
    /* run_bfs's and run_dfs's own checks, in their order: identifiers, the table, then the statement of each direction it follows */
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
        vt->base.zErrMsg = sqlite3_mprintf("%s: traversal failed (check table/column names exist)", name);
        return SQLITE_ERROR;
    }
    if (max_depth <= 0 || (!go_forward && !go_reverse)) /* the start node is popped and not expanded (:280-282, :381-383) */
        return mn_tvf_lone_row(c, start);
    mn_graph *g = 0;
    char *err = 0;
    if (mn_sql_load_graph(vt->db, name, edge_table, src_col, dst_col, 0, direction, 0, 0, 0, &g, &c->ids, &c->n_ids, &err) !=
        SQLITE_OK) { /* whatever it says is replaced */
        sqlite3_free(err);
        vt->base.zErrMsg = sqlite3_mprintf("%s: traversal failed (check table/column names exist)", name);
        return SQLITE_ERROR;
    }
    const int n = c->n_ids;
    int seed = -1;
    for (int i = 0; g && i < n; i++)
        if (!strcmp(c->ids[i], start)) {
            seed = i;
            break;
        }
    if (seed < 0) { /* an empty table, or no row names the start node */
        if (g)
            mn_graph_destroy(g);
        return mn_tvf_lone_row(c, start);
    }
    int64_t row_off[2] = {0, 0};
    const int64_t rows = is_dfs ? mn_graph_dfs(g, mn_dir_code(direction), 1, &seed, max_depth, row_off, 0)
                                : mn_graph_bfs(g, mn_dir_code(direction), 1, &seed, max_depth, row_off, 0);
    int rc = rows < 0 ? SQLITE_ERROR : SQLITE_OK;
    if (rc == SQLITE_OK) {
        int *node = (int *)mn_tvf_alloc(c, GB_NODE, rows, sizeof(int)), *depth = (int *)mn_tvf_alloc(c, GB_DEPTH, rows, sizeof(int));
        int *parent = (int *)mn_tvf_alloc(c, GB_PARENT, rows, sizeof(int));
        if (!node || !depth || !parent) {
            mn_graph_destroy(g);
            return SQLITE_NOMEM;
        }
        rc = (is_dfs ? mn_graph_dfs_rows(g, node, depth, parent) : mn_graph_bfs_rows(g, node, depth, parent)) == 0 ? SQLITE_OK : SQLITE_ERROR;
    }
    if (rc != SQLITE_OK)
        vt->base.zErrMsg = sqlite3_mprintf("%s: %s", name, mn_graph_last_error());
    mn_graph_destroy(g);
    if (rc != SQLITE_OK)
        return rc;
    c->n = rows;
    c->eof = rows == 0;
    return SQLITE_OK;
}

static void gb_column(const MnTvfCursor *c, sqlite3_context *ctx, int col) {
    const int *const node = (const int *)c->buf[GB_NODE], *const depth = (const int *)c->buf[GB_DEPTH];
    const int *const parent = (const int *)c->buf[GB_PARENT];
    switch (col) {
    case GB_NODE:
        sqlite3_result_text(ctx, c->lone ? c->lone : c->ids[node[c->pos]], -1, SQLITE_TRANSIENT);
        break;
    case GB_DEPTH:
        sqlite3_result_int(ctx, c->lone ? 0 : depth[c->pos]);
        break;
    case GB_PARENT:
        if (c->lone || parent[c->pos] < 0)
            sqlite3_result_null(ctx);
        else
            sqlite3_result_text(ctx, c->ids[parent[c->pos]], -1, SQLITE_TRANSIENT);
        break;
    default:
        sqlite3_result_null(ctx);
        break;
    }
}

#define GB_SCHEMA                                                                  \
    "CREATE TABLE x("                                                              \
    "  node TEXT, depth INTEGER, parent TEXT,"                                     \
    "  edge_table TEXT HIDDEN, src_col TEXT HIDDEN, dst_col TEXT HIDDEN,"          \
    "  start_node TEXT HIDDEN, max_depth INTEGER HIDDEN, direction TEXT HIDDEN"    \
    ")"

static const MnTvf bfs_tvf = {
    .name = "graph_bfs", .schema = GB_SCHEMA,
    .first_hidden = GB_EDGE_TABLE, .n_hidden = 6, .rule = MN_TVF_IN_LISTED_ORDER, .required_mask = 0, .cost = 1000.0, /* gtrav_best_index (:822-838) */
    .filter = gb_filter, .column = gb_column,
};

static const MnTvf dfs_tvf = { /* the reference's one module with is_dfs set (:1902) */
    .name = "graph_dfs", .schema = GB_SCHEMA,
    .first_hidden = GB_EDGE_TABLE, .n_hidden = 6, .rule = MN_TVF_IN_LISTED_ORDER, .required_mask = 0, .cost = 1000.0,
    .filter = gb_filter, .column = gb_column,
};

int mn_register_traversal_tvfs(sqlite3 *db) { /* the first two of graph_register_tvfs (src/graph_tvf.c:1898-1914) */
    const int rc = mn_tvf_register(db, &bfs_tvf);
    return rc != SQLITE_OK ? rc : mn_tvf_register(db, &dfs_tvf);
}
