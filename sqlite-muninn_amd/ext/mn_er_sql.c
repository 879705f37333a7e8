/*
 * mn_er_sql.c — muninn_extract_er(hnsw_table, name_col, k, dist_threshold, jw_weight, borderline_delta
 *                                 [, chat_model [, edge_betweenness_threshold [, type_guard]]])
 *
 * The reference's entity-resolution function (src/llama_er.h:7-19, src/llama_er.c:114-592) with its middle stages on the
 * device.  The reference compiles it only together with llama.cpp although nothing in it uses a model (chat_model is parsed
 * and ignored, borderline_delta only enters the threshold); here it is part of the plain extension.
 *
 * Conventions kept from the reference: the entities come from the table `entities(entity_id, <name_col>, source)` read by rowid,
 * rowids shared with the hnsw_index table (:161-186); match_threshold = 1 - dist_threshold + borderline_delta (:143); an empty
 * table answers {"clusters":{}} before the index is touched (:190-193); fewer than six arguments is the reference's error text
 * (:115-118); the result is JSON text, keys in entity order, escaped as json_escape escapes (:68-110), marked with subtype 'J' (:573).
 *
 * Stages:
 *   2-3  blocking, candidate pairs, type guard and scoring cascade (:207-332): one call, mn_hnsw_er_edges, on the index's
 *        device.  MUNINN_ER_BLOCKING=exact asks for the exact neighbours under the threshold (mn_hnsw_knn_graph) instead of
 *        the reference's graph search at k + 1.
 *   5    Leiden (:334-440): temp._er_edges is filled in the reference's order, both directions of every edge, and this
 *        extension's own graph_leiden is read back through SQL, so parity follows from that function's parity.
 *        MUNINN_GRAPH_MODE governs it as it governs graph_leiden: from 2 000 nodes on the default partition is the batched
 *        schedule's, not the reference's sequential one.
 *   6    bridge cut (:442-545): graph_edge_betweenness through SQL, edges above the threshold deleted, Leiden again.
 *
 * Replaced: the n_entities x rows strcmp loops that read Leiden's answer back (:402-430, :507-534) by the hash map of
 * mn_nodemap.h; the string-formatted DELETE (:477-482) by a bound statement — the reference's statement breaks on an entity
 * id that contains a quote, so such ids are outside the parity claim.  A NULL name or entity id is an error here; the
 * reference hands it to strdup.  Keys longer than json_escape's 2 KB scratch are written whole, not cut.
 */
#include "../../include/muninn_hip.h"
#include "mn_nodemap.h"
#include "mn_sqlite_abi.h"
#include "mn_vtab_hnsw.h"

#include <math.h>

/* sqlite3_result_subtype (SQLite >= 3.9.0; the call site checks the library's version, as every slot above 162 is checked).
 * This file is the routine's only user, so its slot is declared here, not in mn_sqlite_abi.h: that header's slot list is held, entry
 * for entry, to a fixture recorded before this function existed.  The number is held to a genuine sqlite3ext.h the same way:
 * scripts/gen_er_golden.py measures it into tests/golden/er.json.gz and tests/test_er_sql.py compares. */
#define MN_ER_SLOT_result_subtype 209
#define sqlite3_result_subtype MN_API(MN_ER_SLOT_result_subtype, void (*)(sqlite3_context *, unsigned int))

typedef struct {
    char *p;
    size_t n, cap;
    int oom;
} Buf;

static void buf_put(Buf *b, const void *s, size_t len) {
    if (b->oom)
        return;
    if (b->n + len + 1 > b->cap) {
        size_t nc = b->cap ? b->cap : 256;
        while (nc < b->n + len + 1)
            nc *= 2;
        char *np = (char *)realloc(b->p, nc);
        if (!np) {
            b->oom = 1;
            return;
        }
        b->p = np;
        b->cap = nc;
    }
    memcpy(b->p + b->n, s, len);
    b->n += len;
    b->p[b->n] = '\0';
}

/* a JSON string as the reference writes one: \" \\ \n \r \t, \u00xx for the other control bytes, everything else as it is */
static void buf_json_string(Buf *b, const char *s) {
    buf_put(b, "\"", 1);
    for (; *s; s++) {
        const unsigned char c = (unsigned char)*s;
        char u[8];
        switch (c) {
        case '"': buf_put(b, "\\\"", 2); break;
        case '\\': buf_put(b, "\\\\", 2); break;
        case '\n': buf_put(b, "\\n", 2); break;
        case '\r': buf_put(b, "\\r", 2); break;
        case '\t': buf_put(b, "\\t", 2); break;
        default:
            if (c < 0x20) {
                snprintf(u, sizeof(u), "\\u%04x", c);
                buf_put(b, u, 6);
            } else {
                buf_put(b, s, 1);
            }
        }
    }
    buf_put(b, "\"", 1);
}

typedef struct {
    int n, cap;
    sqlite3_int64 *rowid;
    char **entity_id;
    int *source; /* 0: empty, else 1 + first-seen index of the source string */
    Buf names;   /* the arena mn_hnsw_er_edges takes */
    int64_t *off;
    NodeMap sources;
} Entities;

static void ent_free(Entities *e) {
    for (int i = 0; i < e->n; i++)
        free(e->entity_id[i]);
    free(e->rowid);
    free(e->entity_id);
    free(e->source);
    free(e->names.p);
    free(e->off);
    nm_free(&e->sources);
}

static int ent_grow(Entities *e) {
    if (e->n < e->cap)
        return 0;
    const int nc = e->cap ? e->cap * 2 : 64;
    sqlite3_int64 *r = (sqlite3_int64 *)realloc(e->rowid, (size_t)nc * sizeof(*r));
    if (r)
        e->rowid = r;
    char **id = (char **)realloc(e->entity_id, (size_t)nc * sizeof(*id));
    if (id)
        e->entity_id = id;
    int *s = (int *)realloc(e->source, (size_t)nc * sizeof(*s));
    if (s)
        e->source = s;
    int64_t *o = (int64_t *)realloc(e->off, ((size_t)nc + 1) * sizeof(*o));
    if (o)
        e->off = o;
    if (!r || !id || !s || !o)
        return -1;
    e->cap = nc;
    return 0;
}

/* graph_leiden's answer over temp._er_edges read into cluster[]: communities numbered in the order the rows name them, entities
 * no row names numbered after them in entity order (:377-440).  first_of[] maps an index of `ids` to the first entity with that id,
 * the entity the reference's scan stops at. */
static int read_leiden(sqlite3 *db, NodeMap *ids, int n_ids, const int *first_of, int n, int *cluster, int with_edges, char **err) {
    int next = 0;
    for (int i = 0; i < n; i++)
        cluster[i] = -1;
    if (with_edges) {
        sqlite3_stmt *st = 0;
        if (sqlite3_prepare_v2(db,
                               "SELECT node, community_id FROM graph_leiden WHERE edge_table = '_er_edges' AND src_col = 'src'"
                               " AND dst_col = 'dst' AND weight_col = 'weight'",
                               -1, &st, 0) != SQLITE_OK) {
            *err = sqlite3_mprintf("%s", sqlite3_errmsg(db));
            return -1;
        }
        NodeMap comm; /* community id -> the order it was first seen in: the reference's comm_keys / comm_remap scan */
        nm_init(&comm);
        int bad = 0;
        while (!bad && sqlite3_step(st) == SQLITE_ROW) {
            const char *node = (const char *)sqlite3_column_text(st, 0);
            char key[24];
            snprintf(key, sizeof(key), "%d", sqlite3_column_int(st, 1));
            if (!node)
                continue;
            const int at = nm_get(ids, node);
            if (at < 0)
                bad = 1;
            else if (at < n_ids) { /* (an id no entity has cannot come back; the map would have appended it) */
                const int c = nm_get(&comm, key);
                if (c < 0)
                    bad = 1;
                else {
                    cluster[first_of[at]] = c;
                    if (c >= next)
                        next = c + 1;
                }
            }
        }
        sqlite3_finalize(st);
        nm_free(&comm);
        if (bad) {
            *err = sqlite3_mprintf("out of memory");
            return -1;
        }
    }
    for (int i = 0; i < n; i++)
        if (cluster[i] < 0)
            cluster[i] = next++;
    return 0;
}

static void fn_extract_er(sqlite3_context *ctx, int argc, sqlite3_value **argv) {
    if (argc < 6) {
        sqlite3_result_error(ctx, "muninn_extract_er: requires at least 6 arguments", -1);
        return;
    }
    const char *hnsw_table = (const char *)sqlite3_value_text(argv[0]);
    const char *name_col = (const char *)sqlite3_value_text(argv[1]);
    const int k = sqlite3_value_int(argv[2]);
    const double dist_threshold = sqlite3_value_double(argv[3]);
    const double jw_weight = sqlite3_value_double(argv[4]);
    const double borderline_delta = sqlite3_value_double(argv[5]);
    /* argv[6], chat_model: parsed by the reference and never used (:292) */
    const double eb_threshold = argc > 7 && sqlite3_value_type(argv[7]) != SQLITE_NULL ? sqlite3_value_double(argv[7]) : -1.0;
    const char *type_guard = argc > 8 ? (const char *)sqlite3_value_text(argv[8]) : 0;
    int guard = MN_ER_GUARD_NONE; /* :130-136: any other text means no guard */
    if (type_guard && !strcmp(type_guard, "same_source"))
        guard = MN_ER_GUARD_SAME_SOURCE;
    else if (type_guard && !strcmp(type_guard, "diff_type"))
        guard = MN_ER_GUARD_DIFF_TYPE;
    if (!hnsw_table || !name_col) {
        sqlite3_result_error(ctx, "muninn_extract_er: hnsw_table and name_col required", -1);
        return;
    }
    const double match_threshold = 1.0 - dist_threshold + borderline_delta; /* :143 */
    sqlite3 *db = sqlite3_context_db_handle(ctx);
    char *err = 0;
    Entities E;
    memset(&E, 0, sizeof(E));
    nm_init(&E.sources);
    NodeMap ids;
    nm_init(&ids);
    int *first_of = 0, *cluster = 0;
    mn_er_edge *edges = 0;
    int have_temp = 0;

    /* ── stage 1: the entities (:158-193) ── */
    {
        char *sql = sqlite3_mprintf("SELECT rowid, entity_id, [%s], source FROM [entities]", name_col);
        sqlite3_stmt *st = 0;
        const int rc = sql ? sqlite3_prepare_v2(db, sql, -1, &st, 0) : SQLITE_NOMEM;
        sqlite3_free(sql);
        if (rc != SQLITE_OK) {
            sqlite3_result_error(ctx, sqlite3_errmsg(db), -1);
            goto done;
        }
        while (sqlite3_step(st) == SQLITE_ROW) {
            const char *id = (const char *)sqlite3_column_text(st, 1);
            const char *name = (const char *)sqlite3_column_text(st, 2);
            const int name_len = sqlite3_column_bytes(st, 2);
            const char *src = (const char *)sqlite3_column_text(st, 3);
            if (!id || !name) {
                err = sqlite3_mprintf("muninn_extract_er: entities row %lld has a NULL entity_id or name",
                                      (long long)sqlite3_column_int64(st, 0));
                break;
            }
            if (ent_grow(&E)) {
                err = sqlite3_mprintf("muninn_extract_er: out of memory");
                break;
            }
            const int i = E.n;
            E.rowid[i] = sqlite3_column_int64(st, 0);
            E.entity_id[i] = strdup(id);
            E.source[i] = src && src[0] ? nm_get(&E.sources, src) + 1 : 0;
            E.off[i] = (int64_t)E.names.n;
            buf_put(&E.names, name, strlen(name) < (size_t)name_len ? strlen(name) : (size_t)name_len); /* a C string there: to the first NUL */
            if (!E.entity_id[i] || E.names.oom || (src && src[0] && E.source[i] <= 0)) {
                free(E.entity_id[i]);
                err = sqlite3_mprintf("muninn_extract_er: out of memory");
                break;
            }
            E.n++;
            E.off[E.n] = (int64_t)E.names.n;
        }
        sqlite3_finalize(st);
        if (err)
            goto fail;
    }
    const int n = E.n;
    if (n == 0) {
        sqlite3_result_text(ctx, "{\"clusters\":{}}", -1, SQLITE_STATIC);
        goto done;
    }

    /* ── stages 2 and 3 on the device (:207-332) ── */
    int64_t n_edges = 0;
    {
        char *ierr = 0;
        mn_index *idx = mn_vtab_hnsw_index_of(db, hnsw_table, 0, &ierr);
        if (!idx) {
            err = sqlite3_mprintf("muninn_extract_er: %s", ierr ? ierr : "no index");
            sqlite3_free(ierr);
            goto fail;
        }
        const char *be = getenv("MUNINN_ER_BLOCKING");
        const int blocking = be && !strcmp(be, "exact") ? MN_ER_EXACT : MN_ER_GRAPH;
        if (be && strcmp(be, "exact") && strcmp(be, "graph")) {
            err = sqlite3_mprintf("muninn_extract_er: MUNINN_ER_BLOCKING must be 'graph' or 'exact', got '%s'", be);
            goto fail;
        }
        const size_t cap = (size_t)n * (size_t)((k > 0 && k < 128 ? k : 0) + 1);
        edges = (mn_er_edge *)malloc(cap * sizeof(*edges));
        if (!edges) {
            err = sqlite3_mprintf("muninn_extract_er: out of memory");
            goto fail;
        }
        n_edges = mn_hnsw_er_edges(idx, n, (const int64_t *)E.rowid, (const unsigned char *)E.names.p, E.off, E.source, k, dist_threshold,
                                   jw_weight, match_threshold, guard, blocking, edges, 0);
        if (n_edges < 0) {
            err = sqlite3_mprintf("muninn_extract_er: %s", mn_last_error());
            goto fail;
        }
    }

    /* ── stage 5: Leiden over temp._er_edges (:334-440) ── */
    sqlite3_exec(db, "DROP TABLE IF EXISTS temp._er_edges", 0, 0, 0);
    {
        char *msg = 0;
        if (sqlite3_exec(db, "CREATE TEMP TABLE _er_edges(src TEXT, dst TEXT, weight REAL)", 0, 0, &msg) != SQLITE_OK) {
            err = sqlite3_mprintf("%s", msg ? msg : "failed to create temp table");
            sqlite3_free(msg);
            goto fail;
        }
        have_temp = 1;
        sqlite3_stmt *ins = 0;
        if (sqlite3_prepare_v2(db, "INSERT INTO temp._er_edges(src, dst, weight) VALUES(?, ?, ?)", -1, &ins, 0) != SQLITE_OK) {
            err = sqlite3_mprintf("%s", sqlite3_errmsg(db));
            goto fail;
        }
        for (int64_t e = 0; e < n_edges; e++)
            for (int dir = 0; dir < 2; dir++) { /* the edge, then its reverse (:354-371) */
                sqlite3_bind_text(ins, 1, E.entity_id[dir ? edges[e].r2 : edges[e].r1], -1, SQLITE_STATIC);
                sqlite3_bind_text(ins, 2, E.entity_id[dir ? edges[e].r1 : edges[e].r2], -1, SQLITE_STATIC);
                sqlite3_bind_double(ins, 3, edges[e].weight);
                sqlite3_step(ins);
                sqlite3_reset(ins);
            }
        sqlite3_finalize(ins);
    }
    first_of = (int *)malloc((size_t)n * sizeof(int));
    cluster = (int *)malloc((size_t)n * sizeof(int));
    if (!first_of || !cluster) {
        err = sqlite3_mprintf("muninn_extract_er: out of memory");
        goto fail;
    }
    for (int i = 0; i < n; i++) {
        const int before = ids.n;
        const int at = nm_get(&ids, E.entity_id[i]);
        if (at < 0) {
            err = sqlite3_mprintf("muninn_extract_er: out of memory");
            goto fail;
        }
        if (ids.n > before) /* a new id; a repeated one keeps the entity the reference's scan stops at */
            first_of[at] = i;
    }
    const int n_ids = ids.n;
    {
        char *lerr = 0;
        if (read_leiden(db, &ids, n_ids, first_of, n, cluster, n_edges > 0, &lerr)) {
            err = lerr;
            goto fail;
        }
    }

    /* ── stage 6: the bridge cut (:442-545) ── */
    if (eb_threshold >= 0 && n_edges > 0) {
        sqlite3_stmt *eb = 0, *del = 0;
        if (sqlite3_prepare_v2(db,
                               "SELECT src, dst, centrality FROM graph_edge_betweenness WHERE edge_table = '_er_edges'"
                               " AND src_col = 'src' AND dst_col = 'dst' AND direction = 'both'",
                               -1, &eb, 0) == SQLITE_OK) {
            /* the bridges are collected first: the scan must not see its own deletes */
            int n_br = 0, cap_br = 0;
            char **br = 0; /* src, dst, src, dst, ... */
            int oom = 0;
            while (!oom && sqlite3_step(eb) == SQLITE_ROW) {
                if (!(sqlite3_column_double(eb, 2) > eb_threshold))
                    continue;
                const char *s = (const char *)sqlite3_column_text(eb, 0), *d = (const char *)sqlite3_column_text(eb, 1);
                if (!s || !d)
                    continue;
                if (n_br + 2 > cap_br) {
                    const int nc = cap_br ? cap_br * 2 : 64;
                    char **nb = (char **)realloc(br, (size_t)nc * sizeof(*nb));
                    if (!nb) {
                        oom = 1;
                        break;
                    }
                    br = nb;
                    cap_br = nc;
                }
                br[n_br] = strdup(s);
                br[n_br + 1] = strdup(d);
                if (!br[n_br] || !br[n_br + 1]) {
                    free(br[n_br]);
                    free(br[n_br + 1]);
                    oom = 1;
                    break;
                }
                n_br += 2;
            }
            sqlite3_finalize(eb);
            if (!oom && n_br > 0 &&
                sqlite3_prepare_v2(db, "DELETE FROM temp._er_edges WHERE (src = ?1 AND dst = ?2) OR (src = ?2 AND dst = ?1)", -1, &del, 0) !=
                    SQLITE_OK)
                oom = 1;
            for (int b = 0; b < n_br; b += 2) {
                if (del) {
                    sqlite3_bind_text(del, 1, br[b], -1, SQLITE_STATIC);
                    sqlite3_bind_text(del, 2, br[b + 1], -1, SQLITE_STATIC);
                    sqlite3_step(del);
                    sqlite3_reset(del);
                }
                free(br[b]);
                free(br[b + 1]);
            }
            free(br);
            if (del)
                sqlite3_finalize(del);
            if (oom) {
                err = sqlite3_mprintf("muninn_extract_er: out of memory");
                goto fail;
            }
            if (n_br > 0) { /* Leiden again on what is left (:489-542) */
                char *lerr = 0;
                sqlite3_stmt *probe = 0;
                /* the reference ignores a second run that cannot be prepared; a run over no edges at all names no node */
                int left = 0;
                if (sqlite3_prepare_v2(db, "SELECT 1 FROM temp._er_edges LIMIT 1", -1, &probe, 0) == SQLITE_OK)
                    left = sqlite3_step(probe) == SQLITE_ROW;
                sqlite3_finalize(probe);
                if (read_leiden(db, &ids, n_ids, first_of, n, cluster, left, &lerr)) {
                    err = lerr;
                    goto fail;
                }
            }
        }
    }

    /* ── the JSON (:547-574) ── */
    {
        Buf js;
        memset(&js, 0, sizeof(js));
        buf_put(&js, "{\"clusters\":{", 13);
        for (int i = 0; i < n; i++) {
            char num[24];
            if (i)
                buf_put(&js, ",", 1);
            buf_json_string(&js, E.entity_id[i]);
            const int len = snprintf(num, sizeof(num), ":%d", cluster[i]);
            buf_put(&js, num, (size_t)len);
        }
        buf_put(&js, "}}", 2);
        if (js.oom) {
            free(js.p);
            err = sqlite3_mprintf("muninn_extract_er: out of memory");
            goto fail;
        }
        sqlite3_result_text(ctx, js.p, (int)js.n, free);
        if (sqlite3_libversion_number() >= 3009000)
            sqlite3_result_subtype(ctx, 'J');
    }
    goto done;

fail:
    sqlite3_result_error(ctx, err ? err : "muninn_extract_er: failed", -1);
    sqlite3_free(err);
done:
    if (have_temp)
        sqlite3_exec(db, "DROP TABLE IF EXISTS temp._er_edges", 0, 0, 0);
    free(edges);
    free(first_of);
    free(cluster);
    nm_free(&ids);
    ent_free(&E);
}

int mn_register_er_functions(sqlite3 *db) { /* :596-599 */
    return sqlite3_create_function(db, "muninn_extract_er", -1, SQLITE_UTF8 | SQLITE_DETERMINISTIC, 0, fn_extract_er, 0, 0);
}
