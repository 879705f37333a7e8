/*
 * mn_select_tvf.c — graph_select over libmuninn_hip.so: its descriptor, xFilter and xColumn on the scaffold of mn_tvf.h.
 * Same eponymous table-valued function as the reference (src/graph_select_tvf.c): declared schema, the four hidden columns
 * all required (idxNum is their bitmask, argv compacted in column order, cost 1000 or 1e12: graph_best_index_common,
 * src/graph_common.h:62-96), xFilter's checks in its order — arguments, NULLs, identifiers, the selector's syntax, the load,
 * the evaluation — with its error strings, rows in ascending node index with rowid = position.  The selector is parsed by
 * mn_select_parse (one parser for SQL and Python); the ingest is mn_sql_load_graph with direction 'both' (text ids → first-seen
 * indices, rows with a NULL endpoint skipped); names are resolved through the ids it returns, in program order, so the first
 * unknown name from the left is the one reported; the evaluation is mn_graph_select.
 *
 * A translation unit of its own: the integrated build (oracle/Makefile) links the reference's graph_select_tvf.c, which
 * registers its own graph_select, next to this repository's other extension sources — nothing of theirs refers to this file.
 */
#include "mn_tvf.h"

#include "mn_nodemap.h"

enum { GS_NODE = 0, GS_DEPTH, GS_DIRECTION, GS_EDGE_TABLE }; /* columns; the result slots are node and depth */
#define GS_REQUIRED 0x0F

static const char *const gs_directions[] = {"self", "ancestor", "descendant", "both", "closure", "selected", "selected", "selected"};

static int gs_filter(MnTvfCursor *c, int idxNum, int argc, sqlite3_value **argv) {
    MnTvfVtab *vt = mn_tvf_vtab(c);
    if ((idxNum & GS_REQUIRED) != GS_REQUIRED || argc < 4) {
        vt->base.zErrMsg = sqlite3_mprintf("graph_select: requires edge_table, src_col, dst_col, selector");
        return SQLITE_ERROR;
    }
    const char *edge_table = (const char *)sqlite3_value_text(argv[0]), *src_col = (const char *)sqlite3_value_text(argv[1]);
    const char *dst_col = (const char *)sqlite3_value_text(argv[2]), *selector = (const char *)sqlite3_value_text(argv[3]);
    if (!edge_table || !src_col || !dst_col || !selector) {
        vt->base.zErrMsg = sqlite3_mprintf("graph_select: NULL parameter not allowed");
        return SQLITE_ERROR;
    }
    if (!ident_ok(edge_table) || !ident_ok(src_col) || !ident_ok(dst_col)) {
        vt->base.zErrMsg = sqlite3_mprintf("graph_select: invalid table/column identifier");
        return SQLITE_ERROR;
    }
    mn_select_op *prog = 0;
    int n_ops = 0;
    if (mn_select_parse(selector, &prog, &n_ops) != 0) {
        vt->base.zErrMsg = sqlite3_mprintf("%s", mn_graph_last_error());
        return SQLITE_ERROR;
    }
    mn_graph *g = 0;
    char *err = 0;
    if (mn_sql_load_graph(vt->db, "graph_select", edge_table, src_col, dst_col, 0, "both", 0, 0, 0, &g, &c->ids, &c->n_ids, &err) !=
        SQLITE_OK) {
        /* what it says is prefixed (a failure past the statement, such as a device that is not there, already names the function) */
        vt->base.zErrMsg = sqlite3_mprintf(err && !strncmp(err, "graph_select: ", 14) ? "%s" : "graph_select: %s", err ? err : "failed to load graph");
        sqlite3_free(err);
        mn_host_free(prog);
        return SQLITE_ERROR;
    }
    const int n = c->n_ids;
    if (!g || n == 0) { /* an empty table answers no rows before any name is looked up (src/graph_selector_eval.c:514) */
        if (g)
            mn_graph_destroy(g);
        mn_host_free(prog);
        return SQLITE_OK;
    }
    c->label = gs_directions[prog[n_ops - 1].op];
    int rc = SQLITE_OK;
    NodeMap nm; /* name → index over the ids the load returned: the same first-seen indices */
    nm_init(&nm);
    for (int i = 0; i < n && rc == SQLITE_OK; i++)
        if (nm_get(&nm, c->ids[i]) != i)
            rc = SQLITE_NOMEM;
    for (int i = 0; i < n_ops && rc == SQLITE_OK; i++) {
        if (prog[i].op > MN_SEL_CLOSURE)
            continue;
        char *name = (char *)malloc((size_t)prog[i].name_len + 1);
        if (!name) {
            rc = SQLITE_NOMEM;
            break;
        }
        memcpy(name, selector + prog[i].name_off, (size_t)prog[i].name_len);
        name[prog[i].name_len] = '\0';
        const int before = nm.n;
        const int at = nm_get(&nm, name);
        if (at < 0)
            rc = SQLITE_NOMEM;
        else if (at >= before) { /* the map did not know it */
            char msg[256];
            snprintf(msg, sizeof(msg), "graph_select: node '%s' not found", name);
            vt->base.zErrMsg = sqlite3_mprintf("%s", msg);
            rc = SQLITE_ERROR;
        } else
            prog[i].node = at;
        free(name);
    }
    nm_free(&nm);
    int64_t rows = 0;
    if (rc == SQLITE_OK) {
        int *node = 0, *depth = 0;
        rows = mn_graph_select(g, prog, n_ops, 0);
        if (rows >= 0) {
            node = (int *)mn_tvf_alloc(c, GS_NODE, rows, sizeof(int));
            depth = (int *)mn_tvf_alloc(c, GS_DEPTH, rows, sizeof(int));
            if (!node || !depth)
                rc = SQLITE_NOMEM;
        }
        if (rc == SQLITE_OK && (rows < 0 || mn_graph_select_rows(g, node, depth) != 0)) {
            vt->base.zErrMsg = sqlite3_mprintf("graph_select: %s", mn_graph_last_error());
            rc = SQLITE_ERROR;
        }
    }
    mn_graph_destroy(g);
    mn_host_free(prog);
    if (rc != SQLITE_OK)
        return rc;
    c->n = rows;
    c->eof = rows == 0;
    return SQLITE_OK;
}

static void gs_column(const MnTvfCursor *c, sqlite3_context *ctx, int col) {
    switch (col) {
    case GS_NODE:
        sqlite3_result_text(ctx, c->ids[((const int *)c->buf[GS_NODE])[c->pos]], -1, SQLITE_TRANSIENT);
        break;
    case GS_DEPTH:
        sqlite3_result_int(ctx, ((const int *)c->buf[GS_DEPTH])[c->pos]);
        break;
    case GS_DIRECTION:
        sqlite3_result_text(ctx, c->label, -1, SQLITE_STATIC);
        break;
    default:
        sqlite3_result_null(ctx);
        break;
    }
}

static const MnTvf select_tvf = {
    .name = "graph_select",
    .schema = "CREATE TABLE x("
              "  node TEXT, depth INTEGER, direction TEXT,"
              "  edge_table TEXT HIDDEN, src_col TEXT HIDDEN, dst_col TEXT HIDDEN, selector TEXT HIDDEN"
              ")",
    .first_hidden = GS_EDGE_TABLE, .n_hidden = 4, .rule = MN_TVF_COMPACTED, .required_mask = GS_REQUIRED, .cost = 1000.0,
    .filter = gs_filter, .column = gs_column,
};

int mn_register_select_tvf(sqlite3 *db) { /* graph_select_register_tvf (src/graph_select_tvf.c:301-303) */
    return mn_tvf_register(db, &select_tvf);
}
