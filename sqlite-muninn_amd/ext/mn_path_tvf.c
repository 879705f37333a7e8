/*
 * mn_path_tvf.c — graph_shortest_path over libmuninn_hip.so: its descriptor, xFilter and xColumn on the scaffold of mn_tvf.h.
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
#include "mn_tvf.h"

#include "mn_nodemap.h"

enum { GSP_NODE = 0, GSP_DISTANCE, GSP_PATH_ORDER, GSP_EDGE_TABLE }; /* columns; the result slots are node and distance */

/* the statement either search prepares before it looks at anything (:478-483, :608-614) */
static int gsp_statement_compiles(sqlite3 *db, const char *t, const char *src, const char *dst, const char *w) {
    return w ? mn_sql_compiles(db, "SELECT \"%w\", \"%w\" FROM \"%w\" WHERE \"%w\" = ?", dst, w, t, src)
             : mn_sql_compiles(db, "SELECT \"%w\" FROM \"%w\" WHERE \"%w\" = ?", dst, t, src);
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

static int gsp_mode(void) { /* auto: the library's choice */
    const int mode = mn_env_graph_mode();
    return mode == MN_GRAPH_MODE_EXACT ? MN_SP_REPLAY : mode == MN_GRAPH_MODE_FAST ? MN_SP_FAST : MN_SP_AUTO;
}

static int gsp_filter(MnTvfCursor *c, int idxNum, int argc, sqlite3_value **argv) {
    (void)idxNum;
    MnTvfVtab *vt = mn_tvf_vtab(c);
    static const char *failed = "graph_shortest_path: search failed";
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
    if (!strcmp(start, end)) /* the seed is popped and is the end, whether or not a row names it (:511, :672) */
        return mn_tvf_lone_row(c, start);
    if (!gsp_named(vt->db, edge_table, src_col, dst_col, start, end)) /* nothing is found, and no device is asked */
        return SQLITE_OK;
    mn_graph *g = 0;
    char *err = 0;
    if (mn_sql_load_graph(vt->db, "graph_shortest_path", edge_table, src_col, dst_col, weight_col, "forward", 0, 0, 0, &g, &c->ids,
                          &c->n_ids, &err) != SQLITE_OK) { /* whatever it says is replaced */
        sqlite3_free(err);
        vt->base.zErrMsg = sqlite3_mprintf("%s", failed);
        return SQLITE_ERROR;
    }
    const int n = c->n_ids;
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
        int *node = (int *)mn_tvf_alloc(c, GSP_NODE, rows, sizeof(int));
        double *dist = (double *)mn_tvf_alloc(c, GSP_DISTANCE, rows, sizeof(double));
        if (!node || !dist) {
            mn_graph_destroy(g);
            return SQLITE_NOMEM;
        }
        rc = mn_graph_shortest_paths_rows(g, node, dist) == 0 ? SQLITE_OK : SQLITE_ERROR;
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

static void gsp_column(const MnTvfCursor *c, sqlite3_context *ctx, int col) {
    switch (col) {
    case GSP_NODE:
        sqlite3_result_text(ctx, c->lone ? c->lone : c->ids[((const int *)c->buf[GSP_NODE])[c->pos]], -1, SQLITE_TRANSIENT);
        break;
    case GSP_DISTANCE:
        sqlite3_result_double(ctx, c->lone ? 0.0 : ((const double *)c->buf[GSP_DISTANCE])[c->pos]);
        break;
    case GSP_PATH_ORDER:
        sqlite3_result_int(ctx, (int)c->pos);
        break;
    default:
        sqlite3_result_null(ctx);
        break;
    }
}

static const MnTvf sp_tvf = {
    .name = "graph_shortest_path",
    .schema = "CREATE TABLE x("
              "  node TEXT, distance REAL, path_order INTEGER,"
              "  edge_table TEXT HIDDEN, src_col TEXT HIDDEN, dst_col TEXT HIDDEN,"
              "  start_node TEXT HIDDEN, end_node TEXT HIDDEN, weight_col TEXT HIDDEN"
              ")",
    .first_hidden = GSP_EDGE_TABLE, .n_hidden = 6, .rule = MN_TVF_IN_LISTED_ORDER, .required_mask = 0, .cost = 1000.0, /* gsp_best_index (:1044-1059) */
    .filter = gsp_filter, .column = gsp_column,
};

int mn_register_path_tvf(sqlite3 *db) { /* the third of graph_register_tvfs (src/graph_tvf.c:1898-1914) */
    return mn_tvf_register(db, &sp_tvf);
}
