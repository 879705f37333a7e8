/*
 * mn_graph_tvf.c — graph_components, graph_pagerank (src/graph_tvf.c:1367-1529 and :1719-1889),
 * graph_node_betweenness, graph_edge_betweenness, graph_closeness and graph_degree (src/graph_centrality.c) over
 * libmuninn_hip.so, on the scaffold of mn_tvf.h.  Per function: the reference's declared schema, its xBestIndex rule and cost,
 * its defaults (damping 0.85, 20 iterations, ...), its checks in its order with its error strings, rows in first-seen node
 * order.  The first two read "SELECT src, dst" themselves (read_edges: the C-ABI takes an edge list); the other four load a
 * device graph with mn_sql_load_graph.
 */
#include "mn_tvf.h"

#include "mn_nodemap.h"

/* "SELECT src, dst FROM edge_table": text ids → first-seen indices (src of a row before its dst), rows with a NULL skipped */
static int read_edges(sqlite3 *db, const char *t, const char *sc, const char *dc, NodeMap *nm, int **src, int **dst, long long *ne) {
    char *sql = sqlite3_mprintf("SELECT \"%w\", \"%w\" FROM \"%w\"", sc, dc, t);
    if (!sql)
        return SQLITE_NOMEM;
    sqlite3_stmt *st = 0;
    int rc = sqlite3_prepare_v2(db, sql, -1, &st, 0);
    sqlite3_free(sql);
    if (rc != SQLITE_OK)
        return rc;
    long long n = 0, cap = 1024;
    int *s = (int *)malloc((size_t)cap * sizeof(int)), *d = (int *)malloc((size_t)cap * sizeof(int));
    int oom = !s || !d;
    while (!oom && (rc = sqlite3_step(st)) == SQLITE_ROW) {
        const char *a = (const char *)sqlite3_column_text(st, 0);
        const char *b = (const char *)sqlite3_column_text(st, 1);
        if (!a || !b)
            continue;
        if (n >= cap) {
            int *s2 = (int *)realloc(s, (size_t)cap * 2 * sizeof(int));
            if (s2)
                s = s2;
            int *d2 = s2 ? (int *)realloc(d, (size_t)cap * 2 * sizeof(int)) : 0;
            if (d2)
                d = d2;
            if (!s2 || !d2) {
                oom = 1;
                break;
            }
            cap *= 2;
        }
        int si = nm_get(nm, a); /* (a's text pointer is only valid until the next column call: nm_get copies) */
        b = (const char *)sqlite3_column_text(st, 1);
        int di = b ? nm_get(nm, b) : -1;
        if (si < 0 || di < 0) {
            oom = 1;
            break;
        }
        s[n] = si;
        d[n] = di;
        n++;
    }
    sqlite3_finalize(st);
    if (oom || rc != SQLITE_DONE) { /* a step error is an error, not the end of the rows */
        free(s);
        free(d);
        return oom ? SQLITE_NOMEM : rc;
    }
    *src = s;
    *dst = d;
    *ne = n;
    return SQLITE_OK;
}

/* both functions' first steps: fewer than three arguments answer no rows (:1446-1449), then the identifier check; on success
 * the edge list is read and the node ids are the cursor's.  1 = answered (rc says how), 0 = go on */
static int edge_list(MnTvfCursor *c, int argc, sqlite3_value **argv, int **src, int **dst, long long *ne, int *rc) {
    *rc = SQLITE_OK;
    if (argc < 3)
        return 1;
    const char *t = (const char *)sqlite3_value_text(argv[0]);
    const char *sc = (const char *)sqlite3_value_text(argv[1]);
    const char *dc = (const char *)sqlite3_value_text(argv[2]);
    if (!ident_ok(t) || !ident_ok(sc) || !ident_ok(dc)) {
        c->base.pVtab->zErrMsg = sqlite3_mprintf("%s: invalid table/column identifier", mn_tvf_vtab(c)->def->name);
        *rc = SQLITE_ERROR;
        return 1;
    }
    NodeMap nm;
    nm_init(&nm);
    *rc = read_edges(mn_tvf_vtab(c)->db, t, sc, dc, &nm, src, dst, ne);
    if (*rc != SQLITE_OK) {
        nm_free(&nm);
        return 1;
    }
    free(nm.slots);
    c->ids = nm.ids; /* ownership of the ids moves to the cursor */
    c->n_ids = nm.n;
    return 0;
}

static void node_rows(MnTvfCursor *c) {
    c->n = c->n_ids;
    c->eof = c->n == 0;
}

/* ───────────────────────── graph_components ───────────────────────── */

enum { GC_NODE = 0, GC_ID, GC_SIZE, GC_EDGE_TABLE };

/* which union sequence: the reference's (component_id = its union-find root) for inputs of its own test sizes, parallel
 * hooking beyond (same partition and sizes, id = smallest node index); MUNINN_GRAPH_MODE=exact|fast forces one */
static int components_mode(long long n_edges) {
    switch (mn_env_graph_mode()) {
    case MN_GRAPH_MODE_EXACT: return MN_COMPONENTS_EXACT;
    case MN_GRAPH_MODE_FAST: return MN_COMPONENTS_FAST;
    default: return n_edges > 200000 ? MN_COMPONENTS_FAST : MN_COMPONENTS_EXACT;
    }
}

static int gc_filter(MnTvfCursor *c, int idxNum, int argc, sqlite3_value **argv) {
    (void)idxNum;
    int *src = 0, *dst = 0, rc;
    long long ne = 0;
    if (edge_list(c, argc, argv, &src, &dst, &ne, &rc))
        return rc;
    if (c->n_ids > 0) {
        int *comp_id = (int *)mn_tvf_alloc(c, GC_ID, c->n_ids, sizeof(int));
        int *comp_size = (int *)mn_tvf_alloc(c, GC_SIZE, c->n_ids, sizeof(int));
        if (!comp_id || !comp_size)
            rc = SQLITE_NOMEM;
        else if (mn_graph_components(c->n_ids, ne, src, dst, components_mode(ne), mn_env_device(), comp_id, comp_size, 0) != 0) {
            c->base.pVtab->zErrMsg = sqlite3_mprintf("graph_components: %s", mn_graph_algo_last_error());
            rc = SQLITE_ERROR;
        }
    }
    free(src);
    free(dst);
    if (rc == SQLITE_OK)
        node_rows(c);
    return rc;
}

static void gc_column(const MnTvfCursor *c, sqlite3_context *ctx, int col) {
    switch (col) {
    case GC_NODE: sqlite3_result_text(ctx, c->ids[c->pos], -1, SQLITE_TRANSIENT); break;
    case GC_ID:
    case GC_SIZE: sqlite3_result_int(ctx, ((const int *)c->buf[col])[c->pos]); break;
    default: sqlite3_result_null(ctx); break;
    }
}

static const MnTvf components_tvf = {
    .name = "graph_components",
    .schema = "CREATE TABLE x(node TEXT, component_id INTEGER, component_size INTEGER,"
              " edge_table TEXT HIDDEN, src_col TEXT HIDDEN, dst_col TEXT HIDDEN)",
    .first_hidden = GC_EDGE_TABLE, .n_hidden = 3, .rule = MN_TVF_BY_POSITION, .required_mask = 0x7, .cost = 1000.0,
    .filter = gc_filter, .column = gc_column,
};

/* ───────────────────────── graph_pagerank ───────────────────────── */

enum { GPR_NODE = 0, GPR_RANK, GPR_EDGE_TABLE };

static int gpr_filter(MnTvfCursor *c, int idxNum, int argc, sqlite3_value **argv) {
    (void)idxNum;
    int *src = 0, *dst = 0, rc;
    long long ne = 0;
    double damping = 0.85; /* :1820-1828 */
    int iterations = 20;
    if (argc > 3 && sqlite3_value_type(argv[3]) != SQLITE_NULL)
        damping = sqlite3_value_double(argv[3]);
    if (argc > 4 && sqlite3_value_type(argv[4]) != SQLITE_NULL)
        iterations = sqlite3_value_int(argv[4]);
    if (edge_list(c, argc, argv, &src, &dst, &ne, &rc))
        return rc;
    if (c->n_ids > 0) {
        double *rank = (double *)mn_tvf_alloc(c, 0, c->n_ids, sizeof(double));
        if (!rank)
            rc = SQLITE_NOMEM;
        else if (mn_graph_pagerank(c->n_ids, ne, src, dst, damping, iterations, mn_env_device(), rank, 0) != 0) {
            c->base.pVtab->zErrMsg = sqlite3_mprintf("graph_pagerank: %s", mn_graph_algo_last_error());
            rc = SQLITE_ERROR;
        }
    }
    free(src);
    free(dst);
    if (rc == SQLITE_OK)
        node_rows(c);
    return rc;
}

static void gpr_column(const MnTvfCursor *c, sqlite3_context *ctx, int col) {
    switch (col) {
    case GPR_NODE: sqlite3_result_text(ctx, c->ids[c->pos], -1, SQLITE_TRANSIENT); break;
    case GPR_RANK: sqlite3_result_double(ctx, ((const double *)c->buf[0])[c->pos]); break;
    default: sqlite3_result_null(ctx); break;
    }
}

static const MnTvf pagerank_tvf = {
    .name = "graph_pagerank",
    .schema = "CREATE TABLE x(node TEXT, rank REAL,"
              " edge_table TEXT HIDDEN, src_col TEXT HIDDEN, dst_col TEXT HIDDEN,"
              " damping REAL HIDDEN, iterations INTEGER HIDDEN)",
    .first_hidden = GPR_EDGE_TABLE, .n_hidden = 5, .rule = MN_TVF_BY_POSITION, .required_mask = 0x7, .cost = 1000.0,
    .filter = gpr_filter, .column = gpr_column,
};

int mn_register_graph_tvfs(sqlite3 *db) { /* the order of graph_register_tvfs (src/graph_tvf.c:1898-1914) */
    int rc = mn_tvf_register(db, &components_tvf);
    if (rc == SQLITE_OK)
        rc = mn_tvf_register(db, &pagerank_tvf);
    return rc;
}

/* ───────────────────────── the four centrality functions (src/graph_centrality.c) ───────────────────────── */

/* what their statements share: the hidden columns decoded over the function's defaults, and the graph on the device */
typedef struct {
    const char *direction;
    int normalized, auto_approx;
    mn_graph *g; /* NULL: an empty graph, no rows */
} CenArgs;

/* hidden-column positions: all four declare these in this order; the betweenness pair has auto_approx_threshold next, and
 * timestamp_col, time_start, time_end close the list */
enum { CEN_EDGE_TABLE = 0, CEN_SRC, CEN_DST, CEN_WEIGHT, CEN_NORMALIZED, CEN_DIRECTION, CEN_REST };

static int cen_load(MnTvfCursor *c, int has_approx, int idxNum, int argc, sqlite3_value **argv, CenArgs *a) {
    MnTvfVtab *vt = mn_tvf_vtab(c);
    sqlite3_value *v[MN_TVF_MAX_HIDDEN], **window = v + CEN_REST + has_approx;
    mn_tvf_args(vt->def, idxNum, argc, argv, v);
    if (v[CEN_NORMALIZED])
        a->normalized = sqlite3_value_int(v[CEN_NORMALIZED]);
    if (has_approx && v[CEN_REST])
        a->auto_approx = sqlite3_value_int(v[CEN_REST]);
    if (mn_value_text(v[CEN_DIRECTION]))
        a->direction = mn_value_text(v[CEN_DIRECTION]);
    char *err = 0;
    if (mn_sql_load_graph(vt->db, vt->def->name, mn_value_text(v[CEN_EDGE_TABLE]), mn_value_text(v[CEN_SRC]), mn_value_text(v[CEN_DST]),
                          mn_value_text(v[CEN_WEIGHT]), a->direction, mn_value_text(window[0]), window[1], window[2], &a->g, &c->ids,
                          &c->n_ids, &err) != SQLITE_OK) {
        vt->base.zErrMsg = err ? err : sqlite3_mprintf("%s: failed to load graph", vt->def->name);
        return SQLITE_ERROR;
    }
    return SQLITE_OK;
}

static int cen_failed(MnTvfCursor *c, mn_graph *g) {
    c->base.pVtab->zErrMsg = sqlite3_mprintf("%s: %s", mn_tvf_vtab(c)->def->name, mn_graph_last_error());
    mn_graph_destroy(g);
    return SQLITE_ERROR;
}

/* ───────────────────────── graph_node_betweenness / graph_edge_betweenness (:752-1240) ───────────────────────── */

enum { BET_CB = 0, BET_E_SRC, BET_E_DST, BET_E_C }; /* result slots: node values; the edge rows */

static int nbet_filter(MnTvfCursor *c, int idxNum, int argc, sqlite3_value **argv) {
    CenArgs a = {"forward", 0, 50000, 0}; /* :872-873, :838 */
    if (argc < 3)
        return SQLITE_OK;
    int rc = cen_load(c, 1, idxNum, argc, argv, &a);
    if (rc != SQLITE_OK || !a.g)
        return rc;
    double *cb = (double *)mn_tvf_alloc(c, BET_CB, c->n_ids, sizeof(double));
    if (!cb) {
        mn_graph_destroy(a.g);
        return SQLITE_NOMEM;
    }
    if (mn_graph_betweenness(a.g, mn_dir_code(a.direction), a.auto_approx, a.normalized, cb, 0) != 0)
        return cen_failed(c, a.g);
    mn_graph_destroy(a.g);
    node_rows(c);
    return SQLITE_OK;
}

static void nbet_column(const MnTvfCursor *c, sqlite3_context *ctx, int col) {
    switch (col) {
    case 0: sqlite3_result_text(ctx, c->ids[c->pos], -1, SQLITE_TRANSIENT); break;
    case 1: sqlite3_result_double(ctx, ((const double *)c->buf[BET_CB])[c->pos]); break;
    default: sqlite3_result_null(ctx); break;
    }
}

static int ebet_filter(MnTvfCursor *c, int idxNum, int argc, sqlite3_value **argv) {
    CenArgs a = {"forward", 0, 0, 0}; /* :1082 */
    if (argc < 3)
        return SQLITE_OK;
    int rc = cen_load(c, 1, idxNum, argc, argv, &a);
    if (rc != SQLITE_OK || !a.g)
        return rc;
    const int n = c->n_ids;
    const long long ne = mn_graph_out_edge_count(a.g);
    double *cb = (double *)mn_tvf_alloc(c, BET_CB, n, sizeof(double));
    int *e_src = (int *)mn_tvf_alloc(c, BET_E_SRC, ne, sizeof(int)), *e_dst = (int *)mn_tvf_alloc(c, BET_E_DST, ne, sizeof(int));
    double *e_c = (double *)mn_tvf_alloc(c, BET_E_C, ne, sizeof(double));
    double *eb = (double *)calloc((size_t)n * (size_t)n, sizeof(double)); /* the reference's dense N x N (:1146) */
    int *off = (int *)malloc(((size_t)n + 1) * sizeof(int)), *tgt = (int *)malloc((size_t)(ne ? ne : 1) * sizeof(int));
    if (!cb || !e_src || !e_dst || !e_c || !eb || !off || !tgt)
        rc = SQLITE_NOMEM;
    else if (mn_graph_betweenness(a.g, mn_dir_code(a.direction), a.auto_approx, a.normalized, cb, eb) != 0 ||
             mn_graph_out_lists(a.g, off, tgt) != 0) {
        c->base.pVtab->zErrMsg = sqlite3_mprintf("%s: %s", mn_tvf_vtab(c)->def->name, mn_graph_last_error());
        rc = SQLITE_ERROR;
    } else { /* only edges that exist in GraphData.out, in list order, with a positive value (:1172-1182) */
        long long rows = 0;
        for (int i = 0; i < n; i++)
            for (int x = off[i]; x < off[i + 1]; x++) {
                const double v = eb[(size_t)i * n + tgt[x]];
                if (v > 0.0) {
                    e_src[rows] = i;
                    e_dst[rows] = tgt[x];
                    e_c[rows++] = v;
                }
            }
        c->n = rows;
        c->eof = rows == 0;
    }
    free(off);
    free(tgt);
    free(eb);
    mn_graph_destroy(a.g);
    return rc;
}

static void ebet_column(const MnTvfCursor *c, sqlite3_context *ctx, int col) {
    switch (col) {
    case 0: sqlite3_result_text(ctx, c->ids[((const int *)c->buf[BET_E_SRC])[c->pos]], -1, SQLITE_TRANSIENT); break;
    case 1: sqlite3_result_text(ctx, c->ids[((const int *)c->buf[BET_E_DST])[c->pos]], -1, SQLITE_TRANSIENT); break;
    case 2: sqlite3_result_double(ctx, ((const double *)c->buf[BET_E_C])[c->pos]); break;
    default: sqlite3_result_null(ctx); break;
    }
}

static const MnTvf node_betweenness_tvf = {
    .name = "graph_node_betweenness",
    .schema = "CREATE TABLE x("
              "  node TEXT, centrality REAL,"
              "  edge_table TEXT HIDDEN, src_col TEXT HIDDEN, dst_col TEXT HIDDEN,"
              "  weight_col TEXT HIDDEN, normalized INTEGER HIDDEN,"
              "  direction TEXT HIDDEN, auto_approx_threshold INTEGER HIDDEN,"
              "  timestamp_col TEXT HIDDEN, time_start HIDDEN, time_end HIDDEN"
              ")",
    .first_hidden = 2, .n_hidden = 10, .rule = MN_TVF_COMPACTED, .required_mask = 0x7, .cost = 1000.0,
    .filter = nbet_filter, .column = nbet_column,
};

static const MnTvf edge_betweenness_tvf = {
    .name = "graph_edge_betweenness",
    .schema = "CREATE TABLE x("
              "  src TEXT, dst TEXT, centrality REAL,"
              "  edge_table TEXT HIDDEN, src_col TEXT HIDDEN, dst_col TEXT HIDDEN,"
              "  weight_col TEXT HIDDEN, normalized INTEGER HIDDEN,"
              "  direction TEXT HIDDEN, auto_approx_threshold INTEGER HIDDEN,"
              "  timestamp_col TEXT HIDDEN, time_start HIDDEN, time_end HIDDEN"
              ")",
    .first_hidden = 3, .n_hidden = 10, .rule = MN_TVF_COMPACTED, .required_mask = 0x7, .cost = 1000.0,
    .filter = ebet_filter, .column = ebet_column,
};

int mn_register_betweenness_tvfs(sqlite3 *db) { /* two of centrality_register_tvfs (src/graph_centrality.c:1510-1530) */
    int rc = mn_tvf_register(db, &node_betweenness_tvf);
    if (rc == SQLITE_OK)
        rc = mn_tvf_register(db, &edge_betweenness_tvf);
    return rc;
}

/* ───────────────────────── graph_closeness / graph_degree (:1269-1504 and :544-750) ───────────────────────── */

static int clos_filter(MnTvfCursor *c, int idxNum, int argc, sqlite3_value **argv) {
    CenArgs a = {"forward", 1, 0, 0}; /* :1370-1371, :1331 */
    if (argc < 3)
        return SQLITE_OK;
    int rc = cen_load(c, 0, idxNum, argc, argv, &a);
    if (rc != SQLITE_OK || !a.g)
        return rc;
    double *val = (double *)mn_tvf_alloc(c, 0, c->n_ids, sizeof(double));
    if (!val) {
        mn_graph_destroy(a.g);
        return SQLITE_NOMEM;
    }
    if (mn_graph_closeness(a.g, mn_dir_code(a.direction), a.normalized, val) != 0)
        return cen_failed(c, a.g);
    mn_graph_destroy(a.g);
    node_rows(c);
    return SQLITE_OK;
}

static int degr_filter(MnTvfCursor *c, int idxNum, int argc, sqlite3_value **argv) {
    CenArgs a = {"both", 0, 0, 0}; /* :646-647, :607 */
    if (argc < 3)
        return SQLITE_OK;
    int rc = cen_load(c, 0, idxNum, argc, argv, &a);
    if (rc != SQLITE_OK || !a.g)
        return rc;
    double *val[4]; /* in_degree, out_degree, degree, centrality */
    for (int k = 0; k < 4; k++)
        val[k] = (double *)mn_tvf_alloc(c, k, c->n_ids, sizeof(double));
    if (c->oom) {
        mn_graph_destroy(a.g);
        return SQLITE_NOMEM;
    }
    if (mn_graph_degree(a.g, a.normalized, val[0], val[1], val[2], val[3]) != 0)
        return cen_failed(c, a.g);
    mn_graph_destroy(a.g);
    node_rows(c);
    return SQLITE_OK;
}

/* column 0 is the node, columns 1 … are the result slots that are filled, in order: closeness has one, degree four */
static void cen_column(const MnTvfCursor *c, sqlite3_context *ctx, int col) {
    if (col == 0)
        sqlite3_result_text(ctx, c->ids[c->pos], -1, SQLITE_TRANSIENT);
    else if (col <= MN_TVF_SLOTS && c->buf[col - 1])
        sqlite3_result_double(ctx, ((const double *)c->buf[col - 1])[c->pos]);
    else
        sqlite3_result_null(ctx);
}

static const MnTvf closeness_tvf = {
    .name = "graph_closeness",
    .schema = "CREATE TABLE x("
              "  node TEXT, centrality REAL,"
              "  edge_table TEXT HIDDEN, src_col TEXT HIDDEN, dst_col TEXT HIDDEN,"
              "  weight_col TEXT HIDDEN, normalized INTEGER HIDDEN,"
              "  direction TEXT HIDDEN, timestamp_col TEXT HIDDEN,"
              "  time_start HIDDEN, time_end HIDDEN"
              ")",
    .first_hidden = 2, .n_hidden = 9, .rule = MN_TVF_COMPACTED, .required_mask = 0x7, .cost = 1000.0,
    .filter = clos_filter, .column = cen_column,
};

static const MnTvf degree_tvf = {
    .name = "graph_degree",
    .schema = "CREATE TABLE x("
              "  node TEXT, in_degree REAL, out_degree REAL, degree REAL, centrality REAL,"
              "  edge_table TEXT HIDDEN, src_col TEXT HIDDEN, dst_col TEXT HIDDEN,"
              "  weight_col TEXT HIDDEN, normalized INTEGER HIDDEN,"
              "  direction TEXT HIDDEN, timestamp_col TEXT HIDDEN,"
              "  time_start HIDDEN, time_end HIDDEN"
              ")",
    .first_hidden = 5, .n_hidden = 9, .rule = MN_TVF_COMPACTED, .required_mask = 0x7, .cost = 1000.0,
    .filter = degr_filter, .column = cen_column,
};

int mn_register_centrality_tvfs(sqlite3 *db) { /* the other two of centrality_register_tvfs (src/graph_centrality.c:1510-1530) */
    int rc = mn_tvf_register(db, &degree_tvf);
    if (rc == SQLITE_OK)
        rc = mn_tvf_register(db, &closeness_tvf);
    return rc;
}
