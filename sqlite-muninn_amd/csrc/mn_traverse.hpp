// mn_traverse.hpp — what mn_graph_bfs and mn_graph_dfs have in common on the host: the checks on their arguments, in the
// order both make them, and the (node, depth, parent) rows of the last call.  `who` is the entry point's name.
#pragma once
#include "mn_graph_int.hpp"

#include <cstring>

// the direction, the seed count and pointers, the node count; the algorithm's own limit on list entries comes next ...
inline int trav_check_args(const char *who, const mn_graph *g, int direction, int64_t n_seeds, const int *seeds, const int64_t *row_off,
                           int *use_out, int *use_in) {
    if (graph_direction(who, direction, use_out, use_in))
        return -1;
    if (n_seeds < 0 || (n_seeds > 0 && !seeds) || !row_off) {
        gset_err("%s: bad arguments (n_seeds = %lld)", who, (long long)n_seeds);
        return -1;
    }
    if (g->n > (1 << 26)) {
        gset_err("%s: more than 2^26 nodes (N = %d)", who, g->n);
        return -1;
    }
    return 0;
}

// ... then the lists (a graph loaded for another direction — graph_data_load fills only the lists its direction traverses —
// has no answer here) and the seeds' range
inline int trav_check_seeds(const char *who, const mn_graph *g, int direction, int64_t n_seeds, const int *seeds) {
    if ((direction == 1 && g->e_out == 0 && g->e_in > 0) || (direction == 2 && g->e_in == 0 && g->e_out > 0) ||
        (direction == 0 && g->e_out != g->e_in)) {
        gset_err("%s: the graph does not hold the %s this direction traverses (%lld out entries, %lld in entries)", who,
                 direction == 1 ? "out-lists" : direction == 2 ? "in-lists" : "out- and in-lists", g->e_out, g->e_in);
        return -1;
    }
    for (int64_t i = 0; i < n_seeds; i++)
        if (seeds[i] < 0 || seeds[i] >= g->n) {
            gset_err("%s: seed %lld is node %d, outside 0 .. %d", who, (long long)i, seeds[i], g->n - 1);
            return -1;
        }
    return 0;
}

struct TravRows {
    std::vector<int> node, depth, parent;
    bool valid = false; // the last call succeeded and these are its rows

    void clear() {
        node.clear();
        depth.clear();
        parent.clear();
        valid = false;
    }

    // the answer that needs no launch: the start rows and nothing else (none for no seeds); fills row_off[0 .. n_seeds]
    void seeds_only(int64_t n_seeds, const int *seeds, int64_t *row_off) {
        node.assign(seeds, seeds + n_seeds);
        depth.assign((size_t)n_seeds, 0);
        parent.assign((size_t)n_seeds, -1);
        for (int64_t i = 0; i <= n_seeds; i++)
            row_off[i] = i;
        valid = true;
    }

    // a chunk's `n` rows from three device columns, behind the rows held: queued on `st`, the caller waits
    int append(hipStream_t st, size_t n, const int *d_node, const int *d_depth, const int *d_parent) {
        const size_t at = node.size();
        node.resize(at + n);
        depth.resize(at + n);
        parent.resize(at + n);
        GCHK(hipMemcpyAsync(node.data() + at, d_node, n * sizeof(int), hipMemcpyDeviceToHost, st));
        GCHK(hipMemcpyAsync(depth.data() + at, d_depth, n * sizeof(int), hipMemcpyDeviceToHost, st));
        GCHK(hipMemcpyAsync(parent.data() + at, d_parent, n * sizeof(int), hipMemcpyDeviceToHost, st));
        return 0;
    }
};

// mn_graph_*_rows: the columns the caller wants of `r`, the rows of the last `who`
inline int trav_rows_out(const TravRows *r, const char *who, int *node, int *depth, int *parent) {
    if (!r || !r->valid) {
        gset_err("%s_rows: no rows (the last %s on this graph failed, or there was none)", who, who);
        return -1;
    }
    const size_t bytes = r->node.size() * sizeof(int);
    if (bytes) {
        if (node)
            memcpy(node, r->node.data(), bytes);
        if (depth)
            memcpy(depth, r->depth.data(), bytes);
        if (parent)
            memcpy(parent, r->parent.data(), bytes);
    }
    return 0;
}
