/*
 * mn_tvf.h — the scaffold of the eponymous table-valued functions, graph_* and hnsw_* (mn_tvf.c): one vtab, one cursor, one sqlite3_module.
 * A function is a descriptor (MnTvf) plus its xFilter and xColumn bodies; everything else — connect, the three xBestIndex
 * rules the reference uses, open / close / next / eof / rowid, freeing what a statement owned — is here once.
 * Exported names carry mn_: the integrated build (oracle/Makefile) links these files next to the reference's own.
 */
#ifndef MN_TVF_H
#define MN_TVF_H

#include "../../include/muninn_hip.h"
#include "mn_sqlite_abi.h"

#include <stddef.h>

/* how xBestIndex hands the hidden-column constraints (usable, =) to xFilter; which function follows which is the reference's */
enum {
    MN_TVF_IN_LISTED_ORDER = 1, /* argvIndex counts up in the order SQLite lists them, whatever the column (gtrav_best_index) */
    MN_TVF_BY_POSITION,         /* argvIndex = hidden-column position + 1, not compacted: a gap is "xBestIndex malfunction" */
    MN_TVF_COMPACTED,           /* argv in column order without gaps, idxNum = bitmask of the columns present
                                   (graph_best_index_common, src/graph_common.h:62-96); decoded by mn_tvf_args */
};

#define MN_TVF_SLOTS 5
#define MN_TVF_MAX_HIDDEN 10

typedef struct MnTvf MnTvf;

typedef struct {
    sqlite3_vtab base;
    sqlite3 *db;
    const MnTvf *def;
} MnTvfVtab;

typedef struct {
    sqlite3_vtab_cursor base;
    char **ids; /* node ids, first-seen order (owned, malloc'ed strings) */
    int n_ids;
    void *buf[MN_TVF_SLOTS]; /* result arrays (owned; mn_tvf_alloc) */
    char *lone;              /* the text of an answer that is one row naming one node (owned; mn_tvf_lone_row) */
    long long n, pos;        /* rows, and the current one: rowid = pos unless the descriptor has a rowid of its own */
    int eof, oom;
    int k;             /* hnsw_*: the width of a group of the [groups][k] answer */
    double q;          /* graph_leiden: the partition's modularity */
    const char *label; /* graph_select: the direction column, a static string */
} MnTvfCursor;

struct MnTvf {
    const char *name, *schema;
    int first_hidden, n_hidden; /* column index of the first hidden column, and how many follow */
    int rule;                   /* MN_TVF_* above */
    int required_mask;          /* hidden columns (bit = position) without which the plan costs 1e12 */
    double cost;                /* the plan's cost with them */
    int (*filter)(MnTvfCursor *c, int idxNum, int argc, sqlite3_value **argv); /* on a cleared cursor */
    void (*column)(const MnTvfCursor *c, sqlite3_context *ctx, int col);
    long long (*rowid)(const MnTvfCursor *c); /* optional: NULL means pos */
};

int mn_tvf_register(sqlite3 *db, const MnTvf *def);

static inline MnTvfVtab *mn_tvf_vtab(MnTvfCursor *c) { return (MnTvfVtab *)c->base.pVtab; }

/* The only way a filter obtains a result array: count elements, zeroed, owned by the cursor's slot.  NULL when memory is out,
 * which the cursor remembers: the statement then fails with SQLITE_NOMEM whatever the filter goes on to return. */
void *mn_tvf_alloc(MnTvfCursor *c, int slot, long long count, size_t elem_size);

/* MN_TVF_COMPACTED's other half: argv scattered by hidden-column position, NULL where the statement gave none */
void mn_tvf_args(const MnTvf *def, int idxNum, int argc, sqlite3_value **argv, sqlite3_value *by_col[MN_TVF_MAX_HIDDEN]);

/* the answer is one row whose node is `text` (copied) */
int mn_tvf_lone_row(MnTvfCursor *c, const char *text);

const char *mn_value_text(sqlite3_value *v); /* graph_safe_text: NULL for an absent or NULL value */
int mn_dir_code(const char *direction);      /* the C-ABI's direction: "both" 0, "reverse" 2, anything else 1 (forward) */

enum { MN_GRAPH_MODE_AUTO = 0, MN_GRAPH_MODE_EXACT, MN_GRAPH_MODE_FAST };
/* MUNINN_GRAPH_MODE: exact → the reference's sequential semantics, fast → the batch-synchronous schedules, unset or anything
 * else → auto, where each caller has its own size threshold */
int mn_env_graph_mode(void);

/* whether the statement mn_sql_compiles(db, "format", ...) spells with sqlite3_mprintf's formats compiles */
int mn_sql_compiles_owned(sqlite3 *db, char *sql);
#define mn_sql_compiles(db, ...) mn_sql_compiles_owned(db, sqlite3_mprintf(__VA_ARGS__))

/* Run, or compile into *st, a statement spelt with sqlite3_mprintf: the text is freed here, and a text that could not be
 * allocated is SQLITE_NOMEM.  *st is NULL unless the result is SQLITE_OK. */
int mn_sql_exec_owned(sqlite3 *db, char *sql);
int mn_sql_prepare_owned(sqlite3 *db, char *sql, sqlite3_stmt **st);

/* mn_graph_sql.c: an edge table (or a graph_adjacency table) → device graph + node ids */
int mn_sql_load_graph(sqlite3 *db, const char *who, const char *edge_table, const char *src_col, const char *dst_col,
                      const char *weight_col, const char *direction, const char *ts_col, sqlite3_value *t0, sqlite3_value *t1,
                      mn_graph **g_out, char ***ids_out, int *n_out, char **err);

#endif /* MN_TVF_H */
