/*
 * mn_tvf.c — the one sqlite3_module behind graph_components, graph_pagerank, graph_node_betweenness, graph_edge_betweenness,
 * graph_closeness, graph_degree, graph_leiden, graph_bfs, graph_dfs, graph_shortest_path, graph_select, hnsw_search_batch,
 * hnsw_search_exact and hnsw_knn_graph (mn_tvf.h).  The descriptor travels as the module's pAux; the entry points below read it
 * and never ask which function they serve.  At the end, the statement helpers the table modules share.
 */
#include "mn_tvf.h"

#include <stdlib.h>
#include <string.h>

static int tvf_connect(sqlite3 *db, void *aux, int argc, const char *const *argv, sqlite3_vtab **out, char **err) {
    (void)argc; (void)argv; (void)err;
    const MnTvf *def = (const MnTvf *)aux;
    int rc = sqlite3_declare_vtab(db, def->schema);
    if (rc != SQLITE_OK)
        return rc;
    MnTvfVtab *v = (MnTvfVtab *)sqlite3_malloc((int)sizeof(MnTvfVtab));
    if (!v)
        return SQLITE_NOMEM;
    memset(v, 0, sizeof(*v));
    v->db = db;
    v->def = def;
    *out = &v->base;
    return SQLITE_OK;
}

static int tvf_disconnect(sqlite3_vtab *v) {
    sqlite3_free(v);
    return SQLITE_OK;
}

static void tvf_use(sqlite3_index_info *ii, int constraint, int argv_index) {
    ii->aConstraintUsage[constraint].argvIndex = argv_index;
    ii->aConstraintUsage[constraint].omit = 1;
}

static int tvf_best_index(sqlite3_vtab *v, sqlite3_index_info *ii) {
    const MnTvf *def = ((MnTvfVtab *)v)->def;
    int which[MN_TVF_MAX_HIDDEN], arg = 1, mask = 0;
    for (int j = 0; j < def->n_hidden; j++)
        which[j] = -1;
    for (int i = 0; i < ii->nConstraint; i++) {
        if (!ii->aConstraint[i].usable || ii->aConstraint[i].op != SQLITE_INDEX_CONSTRAINT_EQ)
            continue;
        const int j = ii->aConstraint[i].iColumn - def->first_hidden;
        if (j < 0 || j >= def->n_hidden)
            continue;
        mask |= 1 << j;
        switch (def->rule) {
        case MN_TVF_IN_LISTED_ORDER: tvf_use(ii, i, arg++); break;
        case MN_TVF_BY_POSITION: tvf_use(ii, i, j + 1); break;
        case MN_TVF_COMPACTED: which[j] = i; break; /* handed over below, in column order */
        }
    }
    if (def->rule == MN_TVF_COMPACTED) {
        for (int j = 0; j < def->n_hidden; j++)
            if (which[j] >= 0)
                tvf_use(ii, which[j], arg++);
        ii->idxNum = mask;
    }
    ii->estimatedCost = (mask & def->required_mask) == def->required_mask ? def->cost : 1e12;
    return SQLITE_OK;
}

void mn_tvf_args(const MnTvf *def, int idxNum, int argc, sqlite3_value **argv, sqlite3_value *by_col[MN_TVF_MAX_HIDDEN]) {
    int pos = 0;
    for (int j = 0; j < def->n_hidden; j++)
        by_col[j] = (idxNum & (1 << j)) && pos < argc ? argv[pos++] : 0;
}

static void tvf_clear(MnTvfCursor *c) {
    for (int i = 0; i < c->n_ids; i++)
        free(c->ids[i]);
    free(c->ids);
    c->ids = 0;
    c->n_ids = 0;
    for (int k = 0; k < MN_TVF_SLOTS; k++) {
        free(c->buf[k]);
        c->buf[k] = 0;
    }
    free(c->lone);
    c->lone = 0;
    c->n = c->pos = 0;
    c->eof = 1;
    c->oom = 0;
    c->k = 0;
    c->q = 0.0;
    c->label = 0;
}

static int tvf_open(sqlite3_vtab *v, sqlite3_vtab_cursor **out) {
    (void)v;
    MnTvfCursor *c = (MnTvfCursor *)calloc(1, sizeof(MnTvfCursor));
    if (!c)
        return SQLITE_NOMEM;
    c->eof = 1;
    *out = &c->base;
    return SQLITE_OK;
}

static int tvf_close(sqlite3_vtab_cursor *cur) {
    tvf_clear((MnTvfCursor *)cur);
    free(cur);
    return SQLITE_OK;
}

static int tvf_filter(sqlite3_vtab_cursor *cur, int idxNum, const char *idxStr, int argc, sqlite3_value **argv) {
    (void)idxStr;
    MnTvfCursor *c = (MnTvfCursor *)cur;
    tvf_clear(c);
    int rc = mn_tvf_vtab(c)->def->filter(c, idxNum, argc, argv);
    return c->oom ? SQLITE_NOMEM : rc;
}

static int tvf_next(sqlite3_vtab_cursor *cur) {
    MnTvfCursor *c = (MnTvfCursor *)cur;
    c->pos++;
    c->eof = c->pos >= c->n;
    return SQLITE_OK;
}

static int tvf_eof(sqlite3_vtab_cursor *cur) { return ((MnTvfCursor *)cur)->eof; }

static int tvf_column(sqlite3_vtab_cursor *cur, sqlite3_context *ctx, int col) {
    MnTvfCursor *c = (MnTvfCursor *)cur;
    mn_tvf_vtab(c)->def->column(c, ctx, col);
    return SQLITE_OK;
}

static int tvf_rowid(sqlite3_vtab_cursor *cur, sqlite3_int64 *out) {
    MnTvfCursor *c = (MnTvfCursor *)cur;
    const MnTvf *def = mn_tvf_vtab(c)->def;
    *out = def->rowid ? def->rowid(c) : c->pos;
    return SQLITE_OK;
}

static sqlite3_module tvf_module = {
    .iVersion = 0,
    .xCreate = 0, /* eponymous */
    .xConnect = tvf_connect,
    .xBestIndex = tvf_best_index,
    .xDisconnect = tvf_disconnect,
    .xDestroy = tvf_disconnect,
    .xOpen = tvf_open,
    .xClose = tvf_close,
    .xFilter = tvf_filter,
    .xNext = tvf_next,
    .xEof = tvf_eof,
    .xColumn = tvf_column,
    .xRowid = tvf_rowid,
};

int mn_tvf_register(sqlite3 *db, const MnTvf *def) { return sqlite3_create_module(db, def->name, &tvf_module, (void *)def); }

void *mn_tvf_alloc(MnTvfCursor *c, int slot, long long count, size_t elem_size) {
    free(c->buf[slot]);
    c->buf[slot] = calloc((size_t)(count > 0 ? count : 1), elem_size);
    if (!c->buf[slot])
        c->oom = 1;
    return c->buf[slot];
}

int mn_tvf_lone_row(MnTvfCursor *c, const char *text) {
    size_t len = strlen(text) + 1;
    c->lone = (char *)malloc(len);
    if (!c->lone)
        return SQLITE_NOMEM;
    memcpy(c->lone, text, len);
    c->n = 1;
    c->eof = 0;
    return SQLITE_OK;
}

const char *mn_value_text(sqlite3_value *v) {
    return v && sqlite3_value_type(v) != SQLITE_NULL ? (const char *)sqlite3_value_text(v) : 0;
}

int mn_dir_code(const char *direction) { return !strcmp(direction, "both") ? 0 : !strcmp(direction, "reverse") ? 2 : 1; }

int mn_env_graph_mode(void) {
    const char *e = getenv("MUNINN_GRAPH_MODE");
    if (e && !strcmp(e, "exact"))
        return MN_GRAPH_MODE_EXACT;
    if (e && !strcmp(e, "fast"))
        return MN_GRAPH_MODE_FAST;
    return MN_GRAPH_MODE_AUTO;
}

int mn_sql_compiles_owned(sqlite3 *db, char *sql) {
    if (!sql)
        return 0;
    sqlite3_stmt *st = 0;
    int rc = sqlite3_prepare_v2(db, sql, -1, &st, 0);
    sqlite3_free(sql);
    sqlite3_finalize(st);
    return rc == SQLITE_OK;
}

int mn_sql_exec_owned(sqlite3 *db, char *sql) {
    if (!sql)
        return SQLITE_NOMEM;
    int rc = sqlite3_exec(db, sql, 0, 0, 0);
    sqlite3_free(sql);
    return rc;
}

int mn_sql_prepare_owned(sqlite3 *db, char *sql, sqlite3_stmt **st) {
    *st = 0;
    if (!sql)
        return SQLITE_NOMEM;
    int rc = sqlite3_prepare_v2(db, sql, -1, st, 0);
    sqlite3_free(sql);
    return rc;
}
