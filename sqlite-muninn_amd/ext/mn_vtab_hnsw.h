/*
 * mn_vtab_hnsw.h — what the rest of the extension needs from the `hnsw_index` table module (mn_vtab_hnsw.c).
 */
#ifndef MN_VTAB_HNSW_H
#define MN_VTAB_HNSW_H

#include "../../include/muninn_hip.h"
#include "mn_sqlite_abi.h"

/* The device index behind a live hnsw_index table of this connection, its queued rows applied first, and (dim != NULL) its
 * dimension.  The one place that finds a live table by name, connects it by touching it when this connection has not yet, and
 * flushes its queue.  NULL + *err (sqlite3_mprintf) when there is no such table — a NULL name reads as '' — or the rows fail. */
mn_index *mn_vtab_hnsw_index_of(sqlite3 *db, const char *table, int *dim, char **err);

/* node2vec_train's output step straight into a live hnsw_index: 1 done, 0 not applicable, -1 error + *err */
int mn_vtab_hnsw_fill_from_n2v(sqlite3 *db, const char *table, int n, const int *off, const int *adj, const mn_n2v_params *prm,
                               int *inserted, char **err);

/* mn_hnsw_tvf.c: hnsw_search_batch, hnsw_search_exact and hnsw_knn_graph; mn_register_hnsw_module registers them after the table
 * wherever that file is in the link */
int mn_register_hnsw_tvfs(sqlite3 *db);

#endif /* MN_VTAB_HNSW_H */
