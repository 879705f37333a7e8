/*
 * muninn_ext.c — SQLite loadable-extension entry point.
 *
 * Same entry symbol and contract as the reference (src/muninn.c:42-121): the file is named
 * muninn.so so SQLite derives `sqlite3_muninn_init`; subsystems are registered in a fixed order and
 * the first failure aborts with *pzErrMsg set via sqlite3_mprintf.  Registered here: the
 * hot-path surface of SURVEY §8(b) — `hnsw_index` (+ `hnsw0` alias), `node2vec_train`,
 * `graph_leiden` — and §8 f-4's `graph_components` / `graph_pagerank` / `graph_node_betweenness` / `graph_edge_betweenness` /
 * `graph_degree` / `graph_closeness` (all on the scaffold of mn_tvf.h), the reference's `graph_bfs` and `graph_dfs` (src/graph_tvf.c:230-416; mn_traverse_tvf.c), its
 * `graph_shortest_path` (src/graph_tvf.c:472-753; mn_path_tvf.c), its `graph_select` (src/graph_select_tvf.c;
 * mn_select_tvf.c), its `muninn_extract_er` (src/llama_er.c) and its `graph_adjacency` virtual table (src/graph_adjacency.c;
 * mn_adjacency_vtab.c), each backed by libmuninn_hip.so (include/muninn_hip.h).
 */
#include "mn_sqlite_abi.h"

const sqlite3_api_routines *mn_sqlite_api = 0;

int mn_register_hnsw_module(sqlite3 *db);
int mn_register_graph_functions(sqlite3 *db) __attribute__((weak));
int mn_register_graph_tvfs(sqlite3 *db) __attribute__((weak));
int mn_register_traversal_tvfs(sqlite3 *db) __attribute__((weak));
int mn_register_select_tvf(sqlite3 *db) __attribute__((weak));
int mn_register_path_tvf(sqlite3 *db) __attribute__((weak));
int mn_register_betweenness_tvfs(sqlite3 *db) __attribute__((weak));
int mn_register_centrality_tvfs(sqlite3 *db) __attribute__((weak));
int mn_register_er_functions(sqlite3 *db) __attribute__((weak));
int mn_register_adjacency_module(sqlite3 *db) __attribute__((weak));

/* in the reference's order; a subsystem whose file is not in the link is passed over */
static const struct {
    int (*reg)(sqlite3 *db);
    const char *failure;
} subsystems[] = {
    {mn_register_hnsw_module, "muninn: failed to register hnsw_index module"},
    {mn_register_graph_functions, "muninn: failed to register graph functions"},
    {mn_register_graph_tvfs, "muninn: failed to register graph TVFs"},
    {mn_register_traversal_tvfs, "muninn: failed to register traversal TVFs"},
    {mn_register_select_tvf, "muninn: failed to register graph_select TVF"},
    {mn_register_path_tvf, "muninn: failed to register graph_shortest_path TVF"},
    {mn_register_betweenness_tvfs, "muninn: failed to register centrality TVFs"},
    {mn_register_centrality_tvfs, "muninn: failed to register centrality TVFs"},
    {mn_register_er_functions, "muninn: failed to register entity resolution functions"},
    {mn_register_adjacency_module, "muninn: failed to register graph_adjacency module"},
};

#ifdef _WIN32
__declspec(dllexport)
#endif
int sqlite3_muninn_init(sqlite3 *db, char **pzErrMsg, const sqlite3_api_routines *pApi) {
    mn_sqlite_api = pApi;
    for (unsigned i = 0; i < sizeof(subsystems) / sizeof(subsystems[0]); i++) {
        if (!subsystems[i].reg)
            continue;
        int rc = subsystems[i].reg(db);
        if (rc != SQLITE_OK) {
            *pzErrMsg = sqlite3_mprintf("%s", subsystems[i].failure);
            return rc;
        }
    }
    return SQLITE_OK;
}
