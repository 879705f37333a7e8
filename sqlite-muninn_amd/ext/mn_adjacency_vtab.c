/*
 * mn_adjacency_vtab.c — the `graph_adjacency` virtual table (src/graph_adjacency.c): a CSR of an edge table kept in six shadow
 * tables, kept current through three triggers and a delta log, and handed to the graph functions.
 *
 * What is contract and therefore restated to the letter: the arguments and their errors (:87-144), the declared schema with the
 * hidden command column (:1050-1055), the shadow tables and triggers (:150-260), the "{t}_config" keys and values, the block
 * layout (4 096 nodes a block, offsets rebased, targets global: src/graph_csr.c:335-400), the freshness rule (:1011-1034), the
 * scan and point lookup (:1200-1328), the command pattern and its four messages (:1332-1369), rename / shadow names / destroy
 * (:1373-1408, :1166-1178).  A database made here opens under the reference's extension and the other way round.
 *
 * What is this project's own: the full rebuild (:565-637) ingests on the host (text id → first-seen index, mn_nodemap.h) and
 * builds both CSRs on the device (mn_graph_from_edges), reads them back once for the blobs (mn_graph_export_csr) and takes the
 * weighted degrees from mn_graph_degree; the incremental rebuild (:649-1005) keeps the reference's structure and merges each
 * touched block through csr_apply_delta as mn_csr_adapter.c defines it (the device merge).  The graph of the last full rebuild
 * stays on the device: see "residency" below.
 *
 * Quirk that comes with the file format: without weight_col the triggers are created with NEW."NULL" / OLD."NULL" in them
 * (:227); the table builds and reads, and every later INSERT / DELETE / UPDATE on the edge table fails with "no such column:
 * NEW.NULL".  The incremental path is therefore reachable on weighted tables only.
 */
#include "../../include/muninn_hip.h"
#include "mn_nodemap.h"
#include "mn_sqlite_abi.h"
#include "mn_tvf.h" /* mn_sql_exec_owned, mn_sql_prepare_owned */

#include <pthread.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#define ADJ_BLOCK 4096 /* CSR_BLOCK_SIZE, src/graph_csr.h */

typedef struct { /* src/graph_csr.h:27-34, as mn_csr_adapter.c restates it */
    int32_t node_count;
    int32_t edge_count;
    int32_t *offsets;
    int32_t *targets;
    double *weights;
    int has_weights;
} CsrArray;
typedef struct { /* src/graph_csr.h:37-42 */
    int32_t src_idx;
    int32_t dst_idx;
    double weight;
    int op;
} CsrDelta;
int csr_apply_delta(const CsrArray *old_csr, const CsrDelta *deltas, int delta_count, int32_t new_node_count, CsrArray *new_csr);

static void csr_free(CsrArray *c) {
    free(c->offsets);
    free(c->targets);
    free(c->weights);
    memset(c, 0, sizeof(*c));
}

typedef struct {
    sqlite3_vtab base;
    sqlite3 *db;
    char *name, *edge_table, *src_col, *dst_col, *weight_col;
    sqlite3_int64 generation; /* read at connect, counted up by every rebuild of this instance, never re-read (:614, :962) */
} AdjTab;

typedef struct {
    sqlite3_vtab_cursor base;
    sqlite3_stmt *st;
    int eof;
} AdjCur;

enum { AC_NODE = 0, AC_IDX, AC_IN, AC_OUT, AC_WIN, AC_WOUT, AC_COMMAND, AC_COUNT };

static const char *const SHADOWS[6] = {"_config", "_nodes", "_degree", "_csr_fwd", "_csr_rev", "_delta"};

/* ───────────────────────── residency ─────────────────────────
 * One entry per connected instance, keyed by (connection, table name).  It holds a reference on the device graph of the state
 * the shadow tables are in, with the generation that state was written under, the connection's data_version then (it moves
 * when ANOTHER connection commits) and the node ids.  mn_sql_load_graph's fresh branch asks mn_adj_resident before it reads
 * a blob and offers what it loaded to mn_adj_resident_offer when there was nothing.  Dropped on incremental rebuild, rollback,
 * rename, disconnect and destroy.  MUNINN_ADJ_RESIDENT=0 turns it off. */
typedef struct {
    sqlite3 *db;
    char *name;
    mn_graph *g;
    sqlite3_int64 generation, data_version;
    char **ids;
    int n;
} AdjEntry;

static pthread_mutex_t adj_mu = PTHREAD_MUTEX_INITIALIZER;
static AdjEntry *adj_entries;
static int adj_n_entries, adj_cap_entries;

static int resident_on(void) {
    const char *e = getenv("MUNINN_ADJ_RESIDENT");
    return !(e && !strcmp(e, "0"));
}

static AdjEntry *entry_find(sqlite3 *db, const char *name) { /* adj_mu held */
    for (int i = 0; i < adj_n_entries; i++)
        if (adj_entries[i].db == db && !strcmp(adj_entries[i].name, name))
            return &adj_entries[i];
    return 0;
}

static void entry_clear(AdjEntry *e) { /* adj_mu held */
    if (e->g)
        mn_graph_destroy(e->g);
    for (int i = 0; e->ids && i < e->n; i++)
        free(e->ids[i]);
    free(e->ids);
    e->g = 0;
    e->ids = 0;
    e->n = 0;
}

static void entry_add(sqlite3 *db, const char *name) {
    pthread_mutex_lock(&adj_mu);
    if (!entry_find(db, name)) {
        if (adj_n_entries == adj_cap_entries) {
            int nc = adj_cap_entries ? adj_cap_entries * 2 : 8;
            AdjEntry *ne = (AdjEntry *)realloc(adj_entries, (size_t)nc * sizeof(AdjEntry));
            if (ne) {
                adj_entries = ne;
                adj_cap_entries = nc;
            }
        }
        size_t len = strlen(name) + 1;
        char *copy = adj_n_entries < adj_cap_entries ? (char *)malloc(len) : 0;
        if (copy) {
            memcpy(copy, name, len);
            AdjEntry *e = &adj_entries[adj_n_entries++];
            memset(e, 0, sizeof(*e));
            e->db = db;
            e->name = copy;
        }
    }
    pthread_mutex_unlock(&adj_mu);
}

static void entry_drop_graph(sqlite3 *db, const char *name) {
    pthread_mutex_lock(&adj_mu);
    AdjEntry *e = entry_find(db, name);
    if (e)
        entry_clear(e);
    pthread_mutex_unlock(&adj_mu);
}

static void entry_remove(sqlite3 *db, const char *name) {
    pthread_mutex_lock(&adj_mu);
    AdjEntry *e = entry_find(db, name);
    if (e) {
        entry_clear(e);
        free(e->name);
        *e = adj_entries[--adj_n_entries];
    }
    pthread_mutex_unlock(&adj_mu);
}

static sqlite3_int64 one_int(sqlite3 *db, const char *sql, sqlite3_int64 dflt) {
    sqlite3_stmt *st = 0;
    sqlite3_int64 v = dflt;
    if (sqlite3_prepare_v2(db, sql, -1, &st, 0) == SQLITE_OK && sqlite3_step(st) == SQLITE_ROW)
        v = sqlite3_column_int64(st, 0);
    sqlite3_finalize(st);
    return v;
}

static char **ids_copy(char *const *ids, int n) {
    char **out = (char **)calloc((size_t)(n ? n : 1), sizeof(char *));
    for (int i = 0; out && i < n; i++) {
        size_t len = strlen(ids[i]) + 1;
        if (!(out[i] = (char *)malloc(len))) {
            for (int k = 0; k < i; k++)
                free(out[k]);
            free(out);
            return 0;
        }
        memcpy(out[i], ids[i], len);
    }
    return out;
}

static sqlite3_int64 cfg_int(sqlite3 *db, const char *name, const char *key, sqlite3_int64 dflt);

/* the entry takes a reference on g and a copy of ids; generation as the config row has it now */
static void entry_set(sqlite3 *db, const char *name, mn_graph *g, char *const *ids, int n, sqlite3_int64 generation) {
    if (!resident_on() || !g || n <= 0)
        return;
    const sqlite3_int64 dv = one_int(db, "PRAGMA data_version", -1);
    char **copy = ids_copy(ids, n);
    if (!copy)
        return;
    pthread_mutex_lock(&adj_mu);
    AdjEntry *e = entry_find(db, name);
    if (e) {
        entry_clear(e);
        mn_graph_retain(g);
        e->g = g;
        e->ids = copy;
        e->n = n;
        e->generation = generation;
        e->data_version = dv;
        copy = 0;
    }
    pthread_mutex_unlock(&adj_mu);
    for (int i = 0; copy && i < n; i++)
        free(copy[i]);
    free(copy);
}

/* the generation of a servable entry, or -1 */
static sqlite3_int64 entry_servable(sqlite3 *db, const char *name) {
    if (!resident_on())
        return -1;
    const sqlite3_int64 gen = cfg_int(db, name, "generation", -1), dv = one_int(db, "PRAGMA data_version", -2);
    sqlite3_int64 out = -1;
    pthread_mutex_lock(&adj_mu);
    AdjEntry *e = entry_find(db, name);
    if (e && e->g && e->generation == gen && e->data_version == dv)
        out = gen;
    pthread_mutex_unlock(&adj_mu);
    return out;
}

static void connect_instance(sqlite3 *db, const char *name) {
    pthread_mutex_lock(&adj_mu);
    const int have = entry_find(db, name) != 0;
    pthread_mutex_unlock(&adj_mu);
    if (have)
        return;
    char *sql = sqlite3_mprintf("SELECT 1 FROM \"%w\"", name); /* prepared, never stepped: SQLite connects the table */
    sqlite3_stmt *st = 0;
    if (sql && sqlite3_prepare_v2(db, sql, -1, &st, 0) == SQLITE_OK)
        sqlite3_finalize(st);
    sqlite3_free(sql);
}

/* mn_sql_load_graph's hook (weak there): a retained handle and a copy of the ids, or NULL for "load as before".  The caller has
 * found the delta log empty. */
mn_graph *mn_adj_resident(sqlite3 *db, const char *name, char ***ids_out, int *n_out) {
    if (!resident_on())
        return 0;
    connect_instance(db, name);
    if (entry_servable(db, name) < 0)
        return 0;
    mn_graph *g = 0;
    pthread_mutex_lock(&adj_mu);
    AdjEntry *e = entry_find(db, name);
    if (e && e->g) {
        char **copy = ids_copy(e->ids, e->n);
        if (copy) {
            g = e->g;
            mn_graph_retain(g);
            *ids_out = copy;
            *n_out = e->n;
        }
    }
    pthread_mutex_unlock(&adj_mu);
    return g;
}

/* ... and what it loaded from the stored blocks when the entry held nothing */
void mn_adj_resident_offer(sqlite3 *db, const char *name, mn_graph *g, char *const *ids, int n) {
    if (!resident_on())
        return;
    connect_instance(db, name);
    entry_set(db, name, g, ids, n, cfg_int(db, name, "generation", -1));
}

/* ───────────────────────── small SQL helpers (statements: mn_sql_exec_owned, mn_sql_prepare_owned of mn_tvf.h) ───────────────────────── */

static int cfg_set(sqlite3 *db, const char *name, const char *key, const char *value) { /* :275-281 */
    return mn_sql_exec_owned(db, sqlite3_mprintf("INSERT OR REPLACE INTO \"%w_config\"(key, value) VALUES ('%w', '%w')", name, key, value));
}

static int cfg_set_int(sqlite3 *db, const char *name, const char *key, sqlite3_int64 v) {
    char buf[32];
    snprintf(buf, sizeof(buf), "%lld", (long long)v);
    return cfg_set(db, name, key, buf);
}

static sqlite3_int64 cfg_int(sqlite3 *db, const char *name, const char *key, sqlite3_int64 dflt) { /* :289-305: atoll of the text */
    sqlite3_stmt *st;
    if (mn_sql_prepare_owned(db, sqlite3_mprintf("SELECT value FROM \"%w_config\" WHERE key='%w'", name, key), &st) != SQLITE_OK)
        return dflt;
    sqlite3_int64 out = dflt;
    if (sqlite3_step(st) == SQLITE_ROW) {
        const char *v = (const char *)sqlite3_column_text(st, 0);
        if (v)
            out = atoll(v);
    }
    sqlite3_finalize(st);
    return out;
}

static sqlite3_int64 delta_rows(sqlite3 *db, const char *name) {
    sqlite3_stmt *st;
    if (mn_sql_prepare_owned(db, sqlite3_mprintf("SELECT COUNT(*) FROM \"%w_delta\"", name), &st) != SQLITE_OK)
        return 0;
    sqlite3_int64 n = sqlite3_step(st) == SQLITE_ROW ? sqlite3_column_int64(st, 0) : 0;
    sqlite3_finalize(st);
    return n;
}

/* ───────────────────────── arguments (:73-144) ───────────────────────── */

static char *arg_value(const char *v) { /* a leading quote of either kind drops the first and the last character; 255 at most */
    size_t len = strlen(v);
    if (len >= 2 && (v[0] == '\'' || v[0] == '"')) {
        len -= 2;
        if (len > 255)
            len = 255;
        return sqlite3_mprintf("%.*s", (int)len, v + 1);
    }
    return sqlite3_mprintf("%s", v);
}

static void tab_free(AdjTab *t) {
    sqlite3_free(t->name);
    sqlite3_free(t->edge_table);
    sqlite3_free(t->src_col);
    sqlite3_free(t->dst_col);
    sqlite3_free(t->weight_col);
    sqlite3_free(t);
}

static int parse_args(int argc, const char *const *argv, AdjTab *t, char **err) {
    static const struct {
        const char *key;
        size_t len;
    } keys[4] = {{"edge_table=", 11}, {"src_col=", 8}, {"dst_col=", 8}, {"weight_col=", 11}};
    char **slot[4] = {&t->edge_table, &t->src_col, &t->dst_col, &t->weight_col};
    for (int i = 3; i < argc; i++) {
        int k = 0;
        while (k < 4 && strncmp(argv[i], keys[k].key, keys[k].len))
            k++;
        if (k == 4) {
            *err = sqlite3_mprintf("graph_adjacency: unknown parameter '%s'", argv[i]);
            return SQLITE_ERROR;
        }
        sqlite3_free(*slot[k]);
        *slot[k] = arg_value(argv[i] + keys[k].len);
    }
    if (!t->edge_table || !t->src_col || !t->dst_col) {
        *err = sqlite3_mprintf("graph_adjacency: edge_table, src_col, and dst_col are required");
        return SQLITE_ERROR;
    }
    if (!ident_ok(t->edge_table) || !ident_ok(t->src_col) || !ident_ok(t->dst_col)) {
        *err = sqlite3_mprintf("graph_adjacency: invalid table/column identifier");
        return SQLITE_ERROR;
    }
    if (t->weight_col && !ident_ok(t->weight_col)) {
        *err = sqlite3_mprintf("graph_adjacency: invalid weight column identifier");
        return SQLITE_ERROR;
    }
    return SQLITE_OK;
}

/* ───────────────────────── shadow tables and triggers (:150-269) ───────────────────────── */

static int create_shadows(sqlite3 *db, const char *name) {
    static const char *const cols[6] = {
        "(key TEXT PRIMARY KEY, value TEXT)",
        "(idx INTEGER PRIMARY KEY, id TEXT UNIQUE)",
        "(idx INTEGER PRIMARY KEY, in_deg INTEGER, out_deg INTEGER, w_in_deg REAL, w_out_deg REAL)",
        "(block_id INTEGER PRIMARY KEY, offsets BLOB, targets BLOB, weights BLOB)",
        "(block_id INTEGER PRIMARY KEY, offsets BLOB, targets BLOB, weights BLOB)",
        "(rowid INTEGER PRIMARY KEY, src TEXT, dst TEXT, weight REAL, op INTEGER)",
    };
    for (int i = 0; i < 6; i++) {
        int rc = mn_sql_exec_owned(db, sqlite3_mprintf("CREATE TABLE IF NOT EXISTS \"%w%s\" %s", name, SHADOWS[i], cols[i]));
        if (rc != SQLITE_OK)
            return rc;
    }
    return SQLITE_OK;
}

static void drop_shadows(sqlite3 *db, const char *name) {
    for (int i = 0; i < 6; i++)
        mn_sql_exec_owned(db, sqlite3_mprintf("DROP TABLE IF EXISTS \"%w%s\"", name, SHADOWS[i]));
}

static int install_triggers(sqlite3 *db, const AdjTab *t, const char *name) {
    const char *w = t->weight_col ? t->weight_col : "NULL"; /* the quirk: NEW."NULL" (:227) */
    int rc = mn_sql_exec_owned(db, sqlite3_mprintf("CREATE TRIGGER IF NOT EXISTS \"%w_ai\" AFTER INSERT ON \"%w\" BEGIN "
                                                   "INSERT INTO \"%w_delta\"(src, dst, weight, op) "
                                                   "VALUES (NEW.\"%w\", NEW.\"%w\", NEW.\"%w\", 1); END",
                                                   name, t->edge_table, name, t->src_col, t->dst_col, w));
    if (rc != SQLITE_OK)
        return rc;
    rc = mn_sql_exec_owned(db, sqlite3_mprintf("CREATE TRIGGER IF NOT EXISTS \"%w_ad\" AFTER DELETE ON \"%w\" BEGIN "
                                               "INSERT INTO \"%w_delta\"(src, dst, weight, op) "
                                               "VALUES (OLD.\"%w\", OLD.\"%w\", OLD.\"%w\", 2); END",
                                               name, t->edge_table, name, t->src_col, t->dst_col, w));
    if (rc != SQLITE_OK)
        return rc;
    return mn_sql_exec_owned(db, sqlite3_mprintf("CREATE TRIGGER IF NOT EXISTS \"%w_au\" AFTER UPDATE ON \"%w\" BEGIN "
                                                 "INSERT INTO \"%w_delta\"(src, dst, weight, op) "
                                                 "VALUES (OLD.\"%w\", OLD.\"%w\", OLD.\"%w\", 2); "
                                                 "INSERT INTO \"%w_delta\"(src, dst, weight, op) "
                                                 "VALUES (NEW.\"%w\", NEW.\"%w\", NEW.\"%w\", 1); END",
                                                 name, t->edge_table, name, t->src_col, t->dst_col, w, name, t->src_col, t->dst_col, w));
}

static void remove_triggers(sqlite3 *db, const char *name) {
    static const char *const suffix[3] = {"_ai", "_ad", "_au"};
    for (int i = 0; i < 3; i++)
        mn_sql_exec_owned(db, sqlite3_mprintf("DROP TRIGGER IF EXISTS \"%w%s\"", name, suffix[i]));
}

/* ───────────────────────── stored blocks (:342-446) ───────────────────────── */

static int store_block(sqlite3 *db, const char *name, const char *suffix, int block_id, const int32_t *off, int nodes,
                       const int32_t *tgt, const double *w, int edges) {
    sqlite3_stmt *st;
    int rc = mn_sql_prepare_owned(db, sqlite3_mprintf("INSERT OR REPLACE INTO \"%w%s\"(block_id, offsets, targets, weights) VALUES (?, ?, ?, ?)",
                                                      name, suffix), &st);
    if (rc != SQLITE_OK)
        return rc;
    sqlite3_bind_int(st, 1, block_id);
    sqlite3_bind_blob(st, 2, off, (nodes + 1) * (int)sizeof(int32_t), SQLITE_STATIC);
    if (edges > 0 && tgt)
        sqlite3_bind_blob(st, 3, tgt, edges * (int)sizeof(int32_t), SQLITE_STATIC);
    else
        sqlite3_bind_blob(st, 3, "", 0, SQLITE_STATIC);
    if (w && edges > 0)
        sqlite3_bind_blob(st, 4, w, edges * (int)sizeof(double), SQLITE_STATIC);
    else
        sqlite3_bind_null(st, 4);
    rc = sqlite3_step(st);
    sqlite3_finalize(st);
    return rc == SQLITE_DONE ? SQLITE_OK : rc;
}

/* a whole CSR as rows of ADJ_BLOCK nodes: offsets rebased to the block's first entry, targets as they are (:380-416) */
static int store_blocks(sqlite3 *db, const char *name, const char *suffix, int n, const int32_t *off, const int32_t *tgt,
                        const double *w) {
    mn_sql_exec_owned(db, sqlite3_mprintf("DELETE FROM \"%w%s\"", name, suffix));
    if (n <= 0) {
        const int32_t zero = 0;
        return store_block(db, name, suffix, 0, &zero, 0, 0, 0, 0);
    }
    int32_t *boff = (int32_t *)malloc((ADJ_BLOCK + 1) * sizeof(int32_t));
    if (!boff)
        return SQLITE_NOMEM;
    int rc = SQLITE_OK;
    for (int b = 0, start = 0; start < n && rc == SQLITE_OK; b++, start += ADJ_BLOCK) {
        const int count = n - start < ADJ_BLOCK ? n - start : ADJ_BLOCK;
        const int32_t first = off[start], edges = off[start + count] - first;
        for (int i = 0; i <= count; i++)
            boff[i] = off[start + i] - first;
        rc = store_block(db, name, suffix, b, boff, count, tgt + first, w ? w + first : 0, edges);
    }
    free(boff);
    return rc;
}

/* one stored block as csr_deserialize reads it (src/graph_csr.c:122-163); a missing row is an all-zero CsrArray (:430-434) */
static int load_block(sqlite3 *db, const char *name, const char *suffix, int block_id, CsrArray *c) {
    memset(c, 0, sizeof(*c));
    sqlite3_stmt *st;
    int rc = mn_sql_prepare_owned(db, sqlite3_mprintf("SELECT offsets, targets, weights FROM \"%w%s\" WHERE block_id=?", name, suffix), &st);
    if (rc != SQLITE_OK)
        return rc;
    sqlite3_bind_int(st, 1, block_id);
    if (sqlite3_step(st) != SQLITE_ROW) {
        sqlite3_finalize(st);
        return SQLITE_OK;
    }
    const void *ob = sqlite3_column_blob(st, 0);
    const int obytes = sqlite3_column_bytes(st, 0);
    const void *tb = sqlite3_column_blob(st, 1);
    const int tbytes = sqlite3_column_bytes(st, 1);
    const void *wb = sqlite3_column_blob(st, 2);
    const int wbytes = sqlite3_column_bytes(st, 2);
    rc = SQLITE_ERROR;
    if (ob && obytes >= (int)sizeof(int32_t)) {
        c->node_count = obytes / (int)sizeof(int32_t) - 1;
        c->edge_count = tbytes / (int)sizeof(int32_t);
        c->has_weights = wb != 0 && wbytes > 0;
        c->offsets = (int32_t *)malloc((size_t)obytes);
        const int want_t = c->edge_count > 0 && tb, want_w = c->has_weights && c->edge_count > 0;
        if (want_t)
            c->targets = (int32_t *)malloc((size_t)tbytes);
        if (want_w)
            c->weights = (double *)malloc((size_t)wbytes);
        if (c->offsets && (!want_t || c->targets) && (!want_w || c->weights)) {
            memcpy(c->offsets, ob, (size_t)obytes);
            if (want_t)
                memcpy(c->targets, tb, (size_t)tbytes);
            if (want_w)
                memcpy(c->weights, wb, (size_t)wbytes);
            rc = SQLITE_OK;
        } else {
            csr_free(c);
        }
    }
    sqlite3_finalize(st);
    return rc;
}

/* every block of one direction joined as csr_merge_blocks joins them (src/graph_csr.c:402-478): a block brings as many nodes as
 * its offsets say, the first block decides whether there are weights, nodes the blocks do not cover are empty */
static int load_all_blocks(sqlite3 *db, const char *name, const char *suffix, int block_size, int n, CsrArray *out) {
    memset(out, 0, sizeof(*out));
    const int nb = (block_size > 0 && n > 0) ? (n + block_size - 1) / block_size : 0;
    if (nb == 0)
        return load_block(db, name, suffix, 0, out);
    CsrArray *blk = (CsrArray *)calloc((size_t)nb, sizeof(CsrArray));
    if (!blk)
        return SQLITE_NOMEM;
    int rc = SQLITE_OK;
    long long edges = 0;
    for (int b = 0; b < nb && rc == SQLITE_OK; b++) {
        rc = load_block(db, name, suffix, b, &blk[b]);
        edges += blk[b].edge_count;
    }
    if (rc == SQLITE_OK) {
        out->node_count = n;
        out->edge_count = (int32_t)edges;
        out->has_weights = blk[0].has_weights;
        out->offsets = (int32_t *)calloc((size_t)n + 1, sizeof(int32_t));
        if (edges > 0)
            out->targets = (int32_t *)calloc((size_t)edges, sizeof(int32_t));
        if (out->has_weights && edges > 0)
            out->weights = (double *)calloc((size_t)edges, sizeof(double));
        if (!out->offsets || (edges > 0 && !out->targets) || (out->has_weights && edges > 0 && !out->weights)) {
            csr_free(out);
            rc = SQLITE_NOMEM;
        }
    }
    if (rc == SQLITE_OK) {
        int32_t eoff = 0, noff = 0;
        for (int b = 0; b < nb; b++) {
            for (int32_t i = 0; i < blk[b].node_count && noff + i < n; i++)
                out->offsets[noff + i] = blk[b].offsets[i] + eoff;
            if (blk[b].edge_count > 0 && blk[b].targets)
                memcpy(out->targets + eoff, blk[b].targets, (size_t)blk[b].edge_count * sizeof(int32_t));
            if (out->weights && blk[b].weights && blk[b].edge_count > 0)
                memcpy(out->weights + eoff, blk[b].weights, (size_t)blk[b].edge_count * sizeof(double));
            eoff += blk[b].edge_count;
            noff += blk[b].node_count;
        }
        for (int32_t i = noff < n ? noff : n; i <= n; i++)
            out->offsets[i] = eoff;
    }
    for (int b = 0; b < nb; b++)
        csr_free(&blk[b]);
    free(blk);
    return rc;
}

/* ───────────────────────── node registry and degrees (:488-559) ───────────────────────── */

static int store_nodes(sqlite3 *db, const char *name, char *const *ids, int n) {
    mn_sql_exec_owned(db, sqlite3_mprintf("DELETE FROM \"%w_nodes\"", name));
    sqlite3_stmt *st;
    int rc = mn_sql_prepare_owned(db, sqlite3_mprintf("INSERT INTO \"%w_nodes\"(idx, id) VALUES (?, ?)", name), &st);
    if (rc != SQLITE_OK)
        return rc;
    for (int i = 0; i < n; i++) {
        sqlite3_bind_int(st, 1, i);
        sqlite3_bind_text(st, 2, ids[i], -1, SQLITE_STATIC);
        sqlite3_step(st);
        sqlite3_reset(st);
    }
    sqlite3_finalize(st);
    return SQLITE_OK;
}

/* counts from the offsets; the weighted sums are the caller's (list-order f64 sums, or the counts where there are no weights) */
static int store_degrees(sqlite3 *db, const char *name, int n, const int32_t *off_out, const int32_t *off_in, const double *w_in,
                         const double *w_out) {
    mn_sql_exec_owned(db, sqlite3_mprintf("DELETE FROM \"%w_degree\"", name));
    sqlite3_stmt *st;
    int rc = mn_sql_prepare_owned(db, sqlite3_mprintf("INSERT INTO \"%w_degree\"(idx, in_deg, out_deg, w_in_deg, w_out_deg) VALUES (?, ?, ?, ?, ?)",
                                                      name), &st);
    if (rc != SQLITE_OK)
        return rc;
    for (int i = 0; i < n; i++) {
        sqlite3_bind_int(st, 1, i);
        sqlite3_bind_int(st, 2, off_in[i + 1] - off_in[i]);
        sqlite3_bind_int(st, 3, off_out[i + 1] - off_out[i]);
        sqlite3_bind_double(st, 4, w_in[i]);
        sqlite3_bind_double(st, 5, w_out[i]);
        sqlite3_step(st);
        sqlite3_reset(st);
    }
    sqlite3_finalize(st);
    return SQLITE_OK;
}

/* ───────────────────────── full rebuild (:565-637) ───────────────────────── */

typedef struct {
    int32_t *s, *d;
    double *w;
    long long n, cap;
} Rows;

static int rows_push(Rows *r, int s, int d, double w, int with_w) {
    if (r->n == r->cap) {
        const long long nc = r->cap ? r->cap * 2 : 1024;
        int32_t *ns = (int32_t *)realloc(r->s, (size_t)nc * sizeof(int32_t));
        if (ns)
            r->s = ns;
        int32_t *nd = (int32_t *)realloc(r->d, (size_t)nc * sizeof(int32_t));
        if (nd)
            r->d = nd;
        double *nw = with_w ? (double *)realloc(r->w, (size_t)nc * sizeof(double)) : 0;
        if (nw)
            r->w = nw;
        if (!ns || !nd || (with_w && !nw))
            return -1;
        r->cap = nc;
    }
    r->s[r->n] = s;
    r->d[r->n] = d;
    if (with_w)
        r->w[r->n] = w;
    r->n++;
    return 0;
}

static int full_rebuild(AdjTab *t) {
    sqlite3 *db = t->db;
    const int with_w = t->weight_col != 0;
    /* graph_data_load's checks and statement (src/graph_load.c:144-198) */
    if (!ident_ok(t->edge_table) || !ident_ok(t->src_col) || !ident_ok(t->dst_col)) {
        t->base.zErrMsg = sqlite3_mprintf("invalid table/column identifier");
        return SQLITE_ERROR;
    }
    if (with_w && !ident_ok(t->weight_col)) {
        t->base.zErrMsg = sqlite3_mprintf("invalid weight column identifier");
        return SQLITE_ERROR;
    }
    sqlite3_stmt *st;
    int rc = mn_sql_prepare_owned(db, with_w ? sqlite3_mprintf("SELECT \"%w\", \"%w\", \"%w\" FROM \"%w\"", t->src_col, t->dst_col, t->weight_col,
                                                               t->edge_table)
                                             : sqlite3_mprintf("SELECT \"%w\", \"%w\" FROM \"%w\"", t->src_col, t->dst_col, t->edge_table), &st);
    if (rc != SQLITE_OK) {
        t->base.zErrMsg = sqlite3_mprintf("failed to prepare: %s", sqlite3_errmsg(db));
        return rc;
    }
    /* ingest on the host: rows with a NULL end are skipped, ids become first-seen indices (:227-246) */
    NodeMap nm;
    nm_init(&nm);
    Rows rows = {0, 0, 0, 0, 0};
    int oom = 0;
    while (!oom && sqlite3_step(st) == SQLITE_ROW) {
        const char *s = (const char *)sqlite3_column_text(st, 0);
        if (!s)
            continue;
        char *scopy = sqlite3_mprintf("%s", s); /* the next column_text may move the first one's bytes */
        const char *d = (const char *)sqlite3_column_text(st, 1);
        if (!d) {
            sqlite3_free(scopy);
            continue;
        }
        const double w = with_w ? sqlite3_column_double(st, 2) : 1.0;
        const int si = scopy ? nm_get(&nm, scopy) : -1;
        const int di = si >= 0 ? nm_get(&nm, d) : -1;
        sqlite3_free(scopy);
        oom = si < 0 || di < 0 || rows_push(&rows, si, di, w, with_w) != 0;
    }
    sqlite3_finalize(st);
    const int n = nm.n;
    int32_t *off[2] = {0, 0}, *tgt[2] = {0, 0};
    double *wts[2] = {0, 0}, *wdeg[2] = {0, 0}; /* [0] out, [1] in */
    mn_graph *g = 0;
    rc = oom ? SQLITE_NOMEM : SQLITE_OK;
    if (rc == SQLITE_OK && n > 0) {
        /* both CSRs on the device (csr_build, src/graph_csr.c:72-83), one read-back for the blobs */
        g = mn_graph_from_edges(n, rows.n, rows.s, rows.d, with_w ? rows.w : 0, 3, mn_env_device());
        if (!g) {
            t->base.zErrMsg = sqlite3_mprintf("graph_adjacency: %s%s", mn_graph_last_error(), mn_env_device_hint());
            rc = SQLITE_ERROR;
        }
        for (int k = 0; k < 2 && rc == SQLITE_OK; k++) {
            off[k] = (int32_t *)malloc(((size_t)n + 1) * sizeof(int32_t));
            tgt[k] = (int32_t *)malloc((size_t)(rows.n ? rows.n : 1) * sizeof(int32_t));
            wdeg[k] = (double *)malloc((size_t)n * sizeof(double));
            if (with_w)
                wts[k] = (double *)malloc((size_t)(rows.n ? rows.n : 1) * sizeof(double));
            if (!off[k] || !tgt[k] || !wdeg[k] || (with_w && !wts[k]))
                rc = SQLITE_NOMEM;
            else if (mn_graph_export_csr(g, k, off[k], tgt[k], wts[k]) < 0) {
                t->base.zErrMsg = sqlite3_mprintf("graph_adjacency: %s", mn_graph_last_error());
                rc = SQLITE_ERROR;
            }
        }
        if (rc == SQLITE_OK && mn_graph_degree(g, 0, wdeg[1], wdeg[0], 0, 0) != 0) {
            t->base.zErrMsg = sqlite3_mprintf("graph_adjacency: %s", mn_graph_last_error());
            rc = SQLITE_ERROR;
        }
    }
    if (rc == SQLITE_OK) {
        sqlite3_exec(db, "SAVEPOINT adj_rebuild", 0, 0, 0);
        rc = store_nodes(db, t->name, nm.ids, n);
        if (rc == SQLITE_OK)
            rc = store_blocks(db, t->name, "_csr_fwd", n, off[0], tgt[0], wts[0]);
        if (rc == SQLITE_OK)
            rc = store_blocks(db, t->name, "_csr_rev", n, off[1], tgt[1], wts[1]);
        if (rc == SQLITE_OK)
            rc = store_degrees(db, t->name, n, off[0], off[1], wdeg[1], wdeg[0]);
        if (rc == SQLITE_OK) {
            t->generation++;
            cfg_set_int(db, t->name, "generation", t->generation);
            cfg_set_int(db, t->name, "node_count", n);
            cfg_set_int(db, t->name, "edge_count", rows.n);
            cfg_set_int(db, t->name, "block_size", ADJ_BLOCK);
            mn_sql_exec_owned(db, sqlite3_mprintf("DELETE FROM \"%w_delta\"", t->name));
        } else {
            sqlite3_exec(db, "ROLLBACK TO adj_rebuild", 0, 0, 0);
        }
        sqlite3_exec(db, "RELEASE adj_rebuild", 0, 0, 0);
    }
    /* the graph stays with the entry (after the savepoint's own xRollbackTo / xRelease callbacks, which drop nothing on success) */
    entry_drop_graph(db, t->name);
    if (rc == SQLITE_OK && g)
        entry_set(db, t->name, g, nm.ids, n, t->generation);
    if (g)
        mn_graph_destroy(g);
    for (int k = 0; k < 2; k++) {
        free(off[k]);
        free(tgt[k]);
        free(wts[k]);
        free(wdeg[k]);
    }
    free(rows.s);
    free(rows.d);
    free(rows.w);
    nm_free(&nm);
    return rc;
}

/* ───────────────────────── incremental rebuild (:649-1005) ───────────────────────── */

/* the blocks a delta list touches by its src_idx, ascending (:649-690) */
static int *touched_blocks(const CsrDelta *dl, int nd, int block_size, int n, int *count) {
    const int nb = (block_size > 0 && n > 0) ? (n + block_size - 1) / block_size : 0;
    char *hit = (char *)calloc((size_t)nb + 1, 1);
    int *ids = (int *)malloc(((size_t)nb + 2) * sizeof(int));
    *count = 0;
    if (!hit || !ids) {
        free(hit);
        free(ids);
        return 0;
    }
    for (int i = 0; i < nd; i++) {
        const int32_t s = dl[i].src_idx;
        if (s >= 0 && s / block_size <= nb)
            hit[s / block_size] = 1;
    }
    for (int b = 0; b <= nb; b++)
        if (hit[b])
            ids[(*count)++] = b;
    free(hit);
    return ids;
}

/* one direction: each touched block is loaded, merged with its slice of the log (src_idx made block-local) and stored.
 * Returns SQLITE_OK, an SQLite error, or -1 when the merge itself failed (the caller then rebuilds in full, :867) */
static int merge_direction(AdjTab *t, const char *suffix, const CsrDelta *dl, int nd, const int *blocks, int n_blocks, int block_size,
                           int new_n) {
    CsrDelta *slice = (CsrDelta *)malloc((size_t)(nd ? nd : 1) * sizeof(CsrDelta));
    if (!slice)
        return -1;
    int rc = SQLITE_OK;
    for (int bi = 0; bi < n_blocks && rc == SQLITE_OK; bi++) {
        const int bid = blocks[bi];
        const int32_t bstart = (int32_t)(bid * block_size);
        int32_t bcount = block_size;
        if (bstart + bcount > new_n)
            bcount = new_n - bstart;
        if (bcount < 0)
            bcount = 0;
        CsrArray old_blk, new_blk;
        rc = load_block(t->db, t->name, suffix, bid, &old_blk);
        if (rc != SQLITE_OK)
            break;
        int ns = 0;
        for (int i = 0; i < nd; i++)
            if (dl[i].src_idx >= bstart && dl[i].src_idx < bstart + bcount) {
                slice[ns] = dl[i];
                slice[ns++].src_idx -= bstart;
            }
        if (csr_apply_delta(&old_blk, slice, ns, bcount, &new_blk) != 0) {
            csr_free(&old_blk);
            rc = -1;
            break;
        }
        csr_free(&old_blk);
        rc = store_block(t->db, t->name, suffix, bid, new_blk.offsets, new_blk.node_count, new_blk.targets,
                         new_blk.has_weights ? new_blk.weights : 0, new_blk.edge_count);
        csr_free(&new_blk);
    }
    free(slice);
    return rc;
}

static void weighted_degrees(const CsrArray *c, int n, double *out) { /* store_degree_one's sums (:693-709) */
    for (int i = 0; i < n; i++) {
        double s = 0.0;
        if (c->has_weights && c->weights)
            for (int32_t j = c->offsets[i]; j < c->offsets[i + 1]; j++)
                s += c->weights[j];
        else
            s = (double)(c->offsets[i + 1] - c->offsets[i]);
        out[i] = s;
    }
}

static int incremental_rebuild(AdjTab *t) {
    sqlite3 *db = t->db;
    const int block_size = (int)cfg_int(db, t->name, "block_size", 0);
    if (block_size <= 0)
        return full_rebuild(t);
    const int32_t old_n = (int32_t)cfg_int(db, t->name, "node_count", 0);
    NodeMap nm;
    nm_init(&nm);
    sqlite3_stmt *st;
    int rc = mn_sql_prepare_owned(db, sqlite3_mprintf("SELECT idx, id FROM \"%w_nodes\" ORDER BY idx", t->name), &st);
    if (rc != SQLITE_OK) {
        nm_free(&nm);
        return rc;
    }
    while (sqlite3_step(st) == SQLITE_ROW) {
        const char *id = (const char *)sqlite3_column_text(st, 1);
        if (id)
            nm_get(&nm, id);
    }
    sqlite3_finalize(st);
    rc = mn_sql_prepare_owned(db, sqlite3_mprintf("SELECT src, dst, weight, op FROM \"%w_delta\"", t->name), &st);
    if (rc != SQLITE_OK) {
        nm_free(&nm);
        return rc;
    }
    CsrDelta *fwd = 0, *rev = 0;
    int nd = 0, cap = 0, oom = 0;
    while (!oom && sqlite3_step(st) == SQLITE_ROW) {
        const char *s = (const char *)sqlite3_column_text(st, 0);
        char *scopy = s ? sqlite3_mprintf("%s", s) : 0;
        const char *d = (const char *)sqlite3_column_text(st, 1);
        const double w = sqlite3_column_double(st, 2);
        const int op = sqlite3_column_int(st, 3);
        if (!s || !d) {
            sqlite3_free(scopy);
            continue;
        }
        const int si = scopy ? nm_get(&nm, scopy) : -1;
        const int di = si >= 0 ? nm_get(&nm, d) : -1;
        sqlite3_free(scopy);
        if (nd == cap) {
            cap = cap ? cap * 2 : 64;
            CsrDelta *nf = (CsrDelta *)realloc(fwd, (size_t)cap * sizeof(CsrDelta));
            if (nf)
                fwd = nf;
            CsrDelta *nr = (CsrDelta *)realloc(rev, (size_t)cap * sizeof(CsrDelta));
            if (nr)
                rev = nr;
            oom = !nf || !nr;
        }
        if (oom || si < 0 || di < 0) {
            oom = 1;
            break;
        }
        memset(&fwd[nd], 0, sizeof(CsrDelta));
        memset(&rev[nd], 0, sizeof(CsrDelta));
        fwd[nd].src_idx = si; fwd[nd].dst_idx = di; fwd[nd].weight = w; fwd[nd].op = op;
        rev[nd].src_idx = di; rev[nd].dst_idx = si; rev[nd].weight = w; rev[nd].op = op;
        nd++;
    }
    sqlite3_finalize(st);
    if (oom || nd == 0) {
        free(fwd);
        free(rev);
        nm_free(&nm);
        return oom ? SQLITE_NOMEM : SQLITE_OK;
    }
    const int32_t new_n = nm.n;
    int nfb = 0, nrb = 0;
    int *fb = touched_blocks(fwd, nd, block_size, new_n, &nfb), *rb = touched_blocks(rev, nd, block_size, new_n, &nrb);
    int full = !fb || !rb; /* :811-819 */
    CsrArray all_fwd, all_rev;
    memset(&all_fwd, 0, sizeof(all_fwd));
    memset(&all_rev, 0, sizeof(all_rev));
    double *w_in = 0, *w_out = 0;
    if (!full) {
        entry_drop_graph(db, t->name); /* the device copy is of the state before this merge */
        sqlite3_exec(db, "SAVEPOINT adj_incr", 0, 0, 0);
        rc = SQLITE_OK;
        if (new_n > old_n)
            rc = store_nodes(db, t->name, nm.ids, new_n);
        if (rc == SQLITE_OK)
            rc = merge_direction(t, "_csr_fwd", fwd, nd, fb, nfb, block_size, new_n);
        if (rc == SQLITE_OK)
            rc = merge_direction(t, "_csr_rev", rev, nd, rb, nrb, block_size, new_n);
        /* the whole degree table again, from the blocks as they now are (:924-960) */
        if (rc == SQLITE_OK)
            rc = load_all_blocks(db, t->name, "_csr_fwd", block_size, new_n, &all_fwd);
        if (rc == SQLITE_OK)
            rc = load_all_blocks(db, t->name, "_csr_rev", block_size, new_n, &all_rev);
        if (rc == SQLITE_OK) {
            w_in = (double *)malloc((size_t)new_n * sizeof(double));
            w_out = (double *)malloc((size_t)new_n * sizeof(double));
            if (!w_in || !w_out || !all_fwd.offsets || !all_rev.offsets || all_fwd.node_count < new_n || all_rev.node_count < new_n)
                rc = SQLITE_NOMEM;
        }
        if (rc == SQLITE_OK) {
            weighted_degrees(&all_fwd, new_n, w_out);
            weighted_degrees(&all_rev, new_n, w_in);
            rc = store_degrees(db, t->name, new_n, all_fwd.offsets, all_rev.offsets, w_in, w_out);
        }
        if (rc == SQLITE_OK) {
            t->generation++;
            cfg_set_int(db, t->name, "generation", t->generation);
            cfg_set_int(db, t->name, "node_count", new_n);
            cfg_set_int(db, t->name, "block_size", block_size);
            sqlite3_int64 net = 0; /* by log rows, not by what the merge found (:967-974) */
            for (int i = 0; i < nd; i++)
                net += fwd[i].op == 1 ? 1 : -1;
            cfg_set_int(db, t->name, "edge_count", cfg_int(db, t->name, "edge_count", 0) + net);
            mn_sql_exec_owned(db, sqlite3_mprintf("DELETE FROM \"%w_delta\"", t->name));
        } else {
            sqlite3_exec(db, "ROLLBACK TO adj_incr", 0, 0, 0);
            full = rc == -1;
        }
        sqlite3_exec(db, "RELEASE adj_incr", 0, 0, 0);
    }
    csr_free(&all_fwd);
    csr_free(&all_rev);
    free(w_in);
    free(w_out);
    free(fwd);
    free(rev);
    free(fb);
    free(rb);
    nm_free(&nm);
    return full ? full_rebuild(t) : rc;
}

static int ensure_fresh(AdjTab *t) { /* :1011-1034 */
    const sqlite3_int64 dc = delta_rows(t->db, t->name);
    if (dc == 0)
        return SQLITE_OK;
    if (cfg_int(t->db, t->name, "generation", 0) == 0)
        return full_rebuild(t);
    sqlite3_int64 limit = cfg_int(t->db, t->name, "edge_count", 0) / 10;
    if (limit < 10)
        limit = 10;
    return dc <= limit ? incremental_rebuild(t) : full_rebuild(t);
}

/* ───────────────────────── the module ───────────────────────── */

static int adj_init(sqlite3 *db, int argc, const char *const *argv, sqlite3_vtab **out, char **err, int create) {
    AdjTab *t = (AdjTab *)sqlite3_malloc((int)sizeof(AdjTab));
    if (!t)
        return SQLITE_NOMEM;
    memset(t, 0, sizeof(*t));
    int rc = parse_args(argc, argv, t, err);
    if (rc == SQLITE_OK) {
        char *schema = sqlite3_mprintf("CREATE TABLE x(node TEXT, node_idx INTEGER, in_degree INTEGER, out_degree INTEGER, "
                                       "weighted_in_degree REAL, weighted_out_degree REAL, \"%w\" HIDDEN)", argv[2]);
        rc = schema ? sqlite3_declare_vtab(db, schema) : SQLITE_NOMEM;
        sqlite3_free(schema);
    }
    if (rc != SQLITE_OK) {
        tab_free(t);
        return rc;
    }
    t->db = db;
    t->name = sqlite3_mprintf("%s", argv[2]);
    if (!create) {
        t->generation = cfg_int(db, argv[2], "generation", 0);
        entry_add(db, t->name);
        *out = &t->base;
        return SQLITE_OK;
    }
    rc = create_shadows(db, argv[2]);
    if (rc != SQLITE_OK) {
        *err = sqlite3_mprintf("graph_adjacency: failed to create shadow tables");
        tab_free(t);
        return rc;
    }
    cfg_set(db, argv[2], "edge_table", t->edge_table);
    cfg_set(db, argv[2], "src_col", t->src_col);
    cfg_set(db, argv[2], "dst_col", t->dst_col);
    if (t->weight_col)
        cfg_set(db, argv[2], "weight_col", t->weight_col);
    cfg_set_int(db, argv[2], "generation", 0);
    rc = install_triggers(db, t, argv[2]);
    if (rc != SQLITE_OK) {
        *err = sqlite3_mprintf("graph_adjacency: failed to install triggers");
        drop_shadows(db, argv[2]);
        tab_free(t);
        return rc;
    }
    entry_add(db, t->name);
    rc = full_rebuild(t);
    if (rc != SQLITE_OK) {
        sqlite3_free(t->base.zErrMsg);
        *err = sqlite3_mprintf("graph_adjacency: initial rebuild failed");
        remove_triggers(db, argv[2]);
        drop_shadows(db, argv[2]);
        entry_remove(db, t->name);
        tab_free(t);
        return rc;
    }
    *out = &t->base;
    return SQLITE_OK;
}

static int adj_create(sqlite3 *db, void *aux, int argc, const char *const *argv, sqlite3_vtab **out, char **err) {
    (void)aux;
    return adj_init(db, argc, argv, out, err, 1);
}
static int adj_connect(sqlite3 *db, void *aux, int argc, const char *const *argv, sqlite3_vtab **out, char **err) {
    (void)aux;
    return adj_init(db, argc, argv, out, err, 0);
}

static int adj_disconnect(sqlite3_vtab *v) {
    AdjTab *t = (AdjTab *)v;
    entry_remove(t->db, t->name);
    tab_free(t);
    return SQLITE_OK;
}

static int adj_destroy(sqlite3_vtab *v) {
    AdjTab *t = (AdjTab *)v;
    remove_triggers(t->db, t->name);
    drop_shadows(t->db, t->name);
    return adj_disconnect(v);
}

static int adj_open(sqlite3_vtab *v, sqlite3_vtab_cursor **out) {
    (void)v;
    AdjCur *c = (AdjCur *)sqlite3_malloc((int)sizeof(AdjCur));
    if (!c)
        return SQLITE_NOMEM;
    memset(c, 0, sizeof(*c));
    *out = &c->base;
    return SQLITE_OK;
}

static int adj_close(sqlite3_vtab_cursor *cur) {
    AdjCur *c = (AdjCur *)cur;
    if (c->st)
        sqlite3_finalize(c->st);
    sqlite3_free(c);
    return SQLITE_OK;
}

static int adj_best_index(sqlite3_vtab *v, sqlite3_index_info *ii) {
    (void)v;
    int eq = -1;
    for (int i = 0; i < ii->nConstraint; i++)
        if (ii->aConstraint[i].usable && ii->aConstraint[i].iColumn == AC_NODE && ii->aConstraint[i].op == SQLITE_INDEX_CONSTRAINT_EQ)
            eq = i;
    if (eq >= 0) {
        ii->idxNum = 1;
        ii->aConstraintUsage[eq].argvIndex = 1;
        ii->aConstraintUsage[eq].omit = 1;
        ii->estimatedCost = 1.0;
        ii->estimatedRows = 1;
    } else {
        ii->idxNum = 0;
        ii->estimatedCost = 1000.0;
        ii->estimatedRows = 1000;
    }
    return SQLITE_OK;
}

static int adj_filter(sqlite3_vtab_cursor *cur, int idxNum, const char *idxStr, int argc, sqlite3_value **argv) {
    (void)idxStr;
    AdjCur *c = (AdjCur *)cur;
    AdjTab *t = (AdjTab *)cur->pVtab;
    if (c->st) {
        sqlite3_finalize(c->st);
        c->st = 0;
    }
    int rc = ensure_fresh(t);
    if (rc != SQLITE_OK)
        return rc;
    const int point = idxNum == 1 && argc >= 1;
    rc = mn_sql_prepare_owned(t->db, sqlite3_mprintf("SELECT n.idx, n.id, COALESCE(d.in_deg, 0), COALESCE(d.out_deg, 0), "
                                                     "COALESCE(d.w_in_deg, 0.0), COALESCE(d.w_out_deg, 0.0) "
                                                     "FROM \"%w_nodes\" n LEFT JOIN \"%w_degree\" d ON n.idx = d.idx %s",
                                                     t->name, t->name, point ? "WHERE n.id = ?" : "ORDER BY n.idx"), &c->st);
    if (rc != SQLITE_OK)
        return rc;
    if (point)
        sqlite3_bind_value(c->st, 1, argv[0]);
    c->eof = sqlite3_step(c->st) != SQLITE_ROW;
    return SQLITE_OK;
}

static int adj_next(sqlite3_vtab_cursor *cur) {
    AdjCur *c = (AdjCur *)cur;
    c->eof = sqlite3_step(c->st) != SQLITE_ROW;
    return SQLITE_OK;
}

static int adj_eof(sqlite3_vtab_cursor *cur) { return ((AdjCur *)cur)->eof; }

static int adj_column(sqlite3_vtab_cursor *cur, sqlite3_context *ctx, int col) {
    AdjCur *c = (AdjCur *)cur;
    static const int from[AC_COMMAND] = {1, 0, 2, 3, 4, 5}; /* node, node_idx, the four degrees */
    if (col < 0 || col >= AC_COMMAND) {
        sqlite3_result_null(ctx);
        return SQLITE_OK;
    }
    const int k = from[col];
    switch (sqlite3_column_type(c->st, k)) {
    case SQLITE_INTEGER: sqlite3_result_int64(ctx, sqlite3_column_int64(c->st, k)); break;
    case SQLITE_FLOAT: sqlite3_result_double(ctx, sqlite3_column_double(c->st, k)); break;
    case SQLITE_TEXT: sqlite3_result_text(ctx, (const char *)sqlite3_column_text(c->st, k), -1, SQLITE_TRANSIENT); break;
    case SQLITE_BLOB: sqlite3_result_blob(ctx, sqlite3_column_blob(c->st, k), sqlite3_column_bytes(c->st, k), SQLITE_TRANSIENT); break;
    default: sqlite3_result_null(ctx); break;
    }
    return SQLITE_OK;
}

static int adj_rowid(sqlite3_vtab_cursor *cur, sqlite3_int64 *out) {
    *out = sqlite3_column_int64(((AdjCur *)cur)->st, 0);
    return SQLITE_OK;
}

static int adj_update(sqlite3_vtab *v, int argc, sqlite3_value **argv, sqlite3_int64 *rowid) { /* :1332-1369 */
    (void)rowid;
    AdjTab *t = (AdjTab *)v;
    if (argc < 2 || sqlite3_value_type(argv[0]) != SQLITE_NULL) {
        v->zErrMsg = sqlite3_mprintf("graph_adjacency: direct INSERT/UPDATE/DELETE not supported; modify the source edge table instead");
        return SQLITE_ERROR;
    }
    const int k = 2 + AC_COMMAND;
    if (k >= argc || sqlite3_value_type(argv[k]) == SQLITE_NULL) {
        v->zErrMsg = sqlite3_mprintf("graph_adjacency: use INSERT INTO t(t) VALUES('rebuild') for commands");
        return SQLITE_ERROR;
    }
    const char *cmd = (const char *)sqlite3_value_text(argv[k]);
    if (!cmd) {
        v->zErrMsg = sqlite3_mprintf("graph_adjacency: NULL command");
        return SQLITE_ERROR;
    }
    if (!strcmp(cmd, "rebuild"))
        return full_rebuild(t);
    if (!strcmp(cmd, "incremental_rebuild"))
        return incremental_rebuild(t);
    if (!strcmp(cmd, "stats"))
        return SQLITE_OK; /* accepted, does nothing */
    v->zErrMsg = sqlite3_mprintf("graph_adjacency: unknown command '%s' (valid: rebuild, incremental_rebuild, stats)", cmd);
    return SQLITE_ERROR;
}

static int adj_rename(sqlite3_vtab *v, const char *to) { /* :1373-1397 */
    AdjTab *t = (AdjTab *)v;
    for (int i = 0; i < 6; i++) {
        int rc = mn_sql_exec_owned(t->db, sqlite3_mprintf("ALTER TABLE \"%w%s\" RENAME TO \"%w%s\"", t->name, SHADOWS[i], to, SHADOWS[i]));
        if (rc != SQLITE_OK)
            return rc;
    }
    remove_triggers(t->db, t->name);
    install_triggers(t->db, t, to);
    entry_remove(t->db, t->name);
    sqlite3_free(t->name);
    t->name = sqlite3_mprintf("%s", to);
    entry_add(t->db, t->name);
    return SQLITE_OK;
}

static int adj_shadow_name(const char *suffix) {
    for (int i = 0; i < 6; i++)
        if (!strcmp(suffix, SHADOWS[i] + 1))
            return 1;
    return 0;
}

/* Transaction callbacks exist for one purpose: SQLite tells the instance when what it wrote is taken back, and the device copy
 * of that state goes.  A rebuild's own SAVEPOINT / RELEASE pass through here too and change nothing. */
static int adj_begin(sqlite3_vtab *v) { (void)v; return SQLITE_OK; }
static int adj_sync(sqlite3_vtab *v) { (void)v; return SQLITE_OK; }
static int adj_commit(sqlite3_vtab *v) { (void)v; return SQLITE_OK; }
static int adj_rollback(sqlite3_vtab *v) {
    entry_drop_graph(((AdjTab *)v)->db, ((AdjTab *)v)->name);
    return SQLITE_OK;
}
static int adj_savepoint(sqlite3_vtab *v, int n) { (void)v; (void)n; return SQLITE_OK; }
static int adj_release(sqlite3_vtab *v, int n) { (void)v; (void)n; return SQLITE_OK; }
static int adj_rollback_to(sqlite3_vtab *v, int n) {
    (void)n;
    return adj_rollback(v);
}

static sqlite3_module adjacency_module = {
    .iVersion = 3,
    .xCreate = adj_create,
    .xConnect = adj_connect,
    .xBestIndex = adj_best_index,
    .xDisconnect = adj_disconnect,
    .xDestroy = adj_destroy,
    .xOpen = adj_open,
    .xClose = adj_close,
    .xFilter = adj_filter,
    .xNext = adj_next,
    .xEof = adj_eof,
    .xColumn = adj_column,
    .xRowid = adj_rowid,
    .xUpdate = adj_update,
    .xBegin = adj_begin,
    .xSync = adj_sync,
    .xCommit = adj_commit,
    .xRollback = adj_rollback,
    .xRename = adj_rename,
    .xSavepoint = adj_savepoint,
    .xRelease = adj_release,
    .xRollbackTo = adj_rollback_to,
    .xShadowName = adj_shadow_name,
};

/* muninn_adjacency_resident(name): the generation of the device copy a graph function would be served, or NULL */
static void fn_resident(sqlite3_context *ctx, int argc, sqlite3_value **argv) {
    (void)argc;
    const char *name = sqlite3_value_type(argv[0]) == SQLITE_NULL ? 0 : (const char *)sqlite3_value_text(argv[0]);
    const sqlite3_int64 gen = name ? entry_servable(sqlite3_context_db_handle(ctx), name) : -1;
    if (gen < 0)
        sqlite3_result_null(ctx);
    else
        sqlite3_result_int64(ctx, gen);
}

int mn_register_adjacency_module(sqlite3 *db) { /* adjacency_register_module, src/graph_adjacency.c:1598-1600 */
    int rc = sqlite3_create_module(db, "graph_adjacency", &adjacency_module, 0);
    if (rc == SQLITE_OK)
        rc = sqlite3_create_function(db, "muninn_adjacency_resident", 1, SQLITE_UTF8, 0, fn_resident, 0, 0);
    return rc;
}
