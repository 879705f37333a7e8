/*
 * mn_select_tvf.c — graph_select over libmuninn_hip.so.
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
#include "../../include/muninn_hip.h"
#include "mn_sqlite_abi.h"

#include "mn_nodemap.h"

int mn_sql_load_graph(sqlite3 *db, const char *who, const char *edge_table, const char *src_col, const char *dst_col,
                      const char *weight_col, const char *direction, const char *ts_col, sqlite3_value *t0, sqlite3_value *t1,
                      mn_graph **g_out, char ***ids_out, int *n_out, char **err); /* mn_graph_sql.c */

typedef struct {
    sqlite3_vtab base;
    sqlite3 *db;
} SelVtab;

typedef struct {
    sqlite3_vtab_cursor base;
    char **ids; /* node ids, first-seen order (owned) */
    int n_ids;
    int *node, *depth;
    const char *direction;
    long long n, pos;
    int eof;
} SelCursor;

enum { GS_NODE = 0, GS_DEPTH, GS_DIRECTION, GS_EDGE_TABLE, GS_SRC, GS_DST, GS_SELECTOR };
#define GS_REQUIRED 0x0F

static const char *const gs_directions[] = {"self", "ancestor", "descendant", "both", "closure", "selected", "selected", "selected"};

static void gs_clear(SelCursor *c) {
    for (int i = 0; i < c->n_ids; i++)
        free(c->ids[i]);
    free(c->ids);
    free(c->node);
    free(c->depth);
    c->ids = 0;
    c->node = c->depth = 0;
    c->n_ids = 0;
    c->n = c->pos = 0;
    c->eof = 1;
}

static int gs_connect(sqlite3 *db, void *aux, int argc, const char *const *argv, sqlite3_vtab **out, char **err) {
    (void)aux; (void)argc; (void)argv; (void)err;
    int rc = sqlite3_declare_vtab(db, "CREATE TABLE x("
                                      "  node TEXT, depth INTEGER, direction TEXT,"
                                      "  edge_table TEXT HIDDEN, src_col TEXT HIDDEN, dst_col TEXT HIDDEN, selector TEXT HIDDEN"
                                      ")");
    if (rc != SQLITE_OK)
        return rc;
    SelVtab *v = (SelVtab *)sqlite3_malloc((int)sizeof(SelVtab));
    if (!v)
        return SQLITE_NOMEM;
    memset(v, 0, sizeof(*v));
    v->db = db;
    *out = &v->base;
    return SQLITE_OK;
}

static int gs_disconnect(sqlite3_vtab *v) {
    sqlite3_free(v);
    return SQLITE_OK;
}

static int gs_best_index(sqlite3_vtab *v, sqlite3_index_info *ii) {
    (void)v;
    int which[4] = {-1, -1, -1, -1};
    for (int i = 0; i < ii->nConstraint; i++) {
        if (!ii->aConstraint[i].usable || ii->aConstraint[i].op != SQLITE_INDEX_CONSTRAINT_EQ)
            continue;
        int col = ii->aConstraint[i].iColumn;
        if (col >= GS_EDGE_TABLE && col <= GS_SELECTOR)
            which[col - GS_EDGE_TABLE] = i;
    }
    int arg = 1, mask = 0;
    for (int j = 0; j < 4; j++)
        if (which[j] >= 0) {
            ii->aConstraintUsage[which[j]].argvIndex = arg++;
            ii->aConstraintUsage[which[j]].omit = 1;
            mask |= 1 << j;
        }
    ii->idxNum = mask;
    ii->estimatedCost = (mask & GS_REQUIRED) == GS_REQUIRED ? 1000.0 : 1e12;
    return SQLITE_OK;
}

static int gs_open(sqlite3_vtab *v, sqlite3_vtab_cursor **out) {
    (void)v;
    SelCursor *c = (SelCursor *)calloc(1, sizeof(SelCursor));
    if (!c)
        return SQLITE_NOMEM;
    c->eof = 1;
    *out = &c->base;
    return SQLITE_OK;
}

static int gs_close(sqlite3_vtab_cursor *cur) {
    gs_clear((SelCursor *)cur);
    free(cur);
    return SQLITE_OK;
}

static int gs_filter(sqlite3_vtab_cursor *cur, int idxNum, const char *idxStr, int argc, sqlite3_value **argv) {
    (void)idxStr;
    SelCursor *c = (SelCursor *)cur;
    SelVtab *vt = (SelVtab *)cur->pVtab;
    gs_clear(c);
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
    int n = 0;
    if (mn_sql_load_graph(vt->db, "graph_select", edge_table, src_col, dst_col, 0, "both", 0, 0, 0, &g, &c->ids, &n, &err) != SQLITE_OK) {
        /* (a failure past the statement, such as a device that is not there, already names the function) */
        vt->base.zErrMsg = sqlite3_mprintf(err && !strncmp(err, "graph_select: ", 14) ? "%s" : "graph_select: %s", err ? err : "failed to load graph");
        sqlite3_free(err);
        mn_host_free(prog);
        return SQLITE_ERROR;
    }
    c->n_ids = n;
    if (!g || n == 0) { /* an empty table answers no rows before any name is looked up (src/graph_selector_eval.c:514) */
        if (g)
            mn_graph_destroy(g);
        mn_host_free(prog);
        return SQLITE_OK;
    }
    c->direction = gs_directions[prog[n_ops - 1].op];
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
        rows = mn_graph_select(g, prog, n_ops, 0);
        if (rows >= 0) {
            c->node = (int *)malloc((size_t)(rows ? rows : 1) * sizeof(int));
            c->depth = (int *)malloc((size_t)(rows ? rows : 1) * sizeof(int));
            if (!c->node || !c->depth)
                rc = SQLITE_NOMEM;
        }
        if (rc == SQLITE_OK && (rows < 0 || mn_graph_select_rows(g, c->node, c->depth) != 0)) {
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

static int gs_next(sqlite3_vtab_cursor *cur) {
    SelCursor *c = (SelCursor *)cur;
    c->pos++;
    c->eof = c->pos >= c->n;
    return SQLITE_OK;
}
static int gs_eof(sqlite3_vtab_cursor *cur) { return ((SelCursor *)cur)->eof; }
static int gs_rowid(sqlite3_vtab_cursor *cur, sqlite3_int64 *out) {
    *out = ((SelCursor *)cur)->pos;
    return SQLITE_OK;
}

static int gs_column(sqlite3_vtab_cursor *cur, sqlite3_context *ctx, int col) {
    SelCursor *c = (SelCursor *)cur;
    switch (col) {
    case GS_NODE:
        sqlite3_result_text(ctx, c->ids[c->node[c->pos]], -1, SQLITE_TRANSIENT);
        break;
    case GS_DEPTH:
        sqlite3_result_int(ctx, c->depth[c->pos]);
        break;
    case GS_DIRECTION:
        sqlite3_result_text(ctx, c->direction, -1, SQLITE_STATIC);
        break;
    default:
        sqlite3_result_null(ctx);
        break;
    }
    return SQLITE_OK;
}

static sqlite3_module select_module = {
    .iVersion = 0, .xCreate = 0, .xConnect = gs_connect, .xBestIndex = gs_best_index, .xDisconnect = gs_disconnect,
    .xDestroy = gs_disconnect, .xOpen = gs_open, .xClose = gs_close, .xFilter = gs_filter, .xNext = gs_next,
    .xEof = gs_eof, .xColumn = gs_column, .xRowid = gs_rowid,
};

int mn_register_select_tvf(sqlite3 *db) { /* graph_select_register_tvf (src/graph_select_tvf.c:301-303) */
    return sqlite3_create_module(db, "graph_select", &select_module, 0);
}
