// mn_select.hip — the reference's lineage selectors (graph_select: src/graph_selector_parse.c, src/graph_selector_eval.c)
// over an mn_graph's device-resident CSR, gfx950:
//   mn_select_parse       selector text → postfix program (host only: no device is touched)
//   mn_graph_select       the program evaluated on the device: a stack machine over n-bit sets
//   mn_graph_select_rows  the (node, depth) rows of the last call, in ascending node index
//
// What the reference computes is a SET of nodes and, per node, a hop distance from a seed set, listed by node index: no
// arrival order enters the answer, so a level-synchronous traversal gives its rows whatever the launch shape.
//
//   reach    from a seed set under a pre-visited set (the nodes already in the result are neither reported nor expanded
//            through: `+x+` runs its descendant pass over the ancestors' visited set).  One launch per level — the kernel
//            boundary is what makes a level's claims visible to the next.  Frontiers are bitmaps, three of them in rotation:
//            level L reads F[(L-1)%3], writes F[L%3] and clears F[(L+1)%3].  A level's kernel takes one of two forms, chosen
//            ON THE DEVICE from the list-entry count of the frontier (cnt[(L-1)%3], summed by the level before):
//              top-down   one wavefront per frontier word; its lanes work over the concatenated list entries of the word's
//                         frontier nodes (prefix sums in LDS, a binary search finds an entry's node).  A node is claimed by
//                         the value atomicOr returns on its visited word; the winner writes the depth and the next
//                         frontier's bit.
//              bottom-up  one wavefront owns the 64 nodes of a word: each unvisited lane scans its node's OPPOSITE list for a
//                         member of the frontier and stops at the first; the ballot is the word of the next frontier and is
//                         OR-ed into the wavefront's own visited word with plain stores.
//            A level whose frontier has no list entries is a no-op, so MN_SELECT_LEVELS_PER_SYNC levels (never past the depth
//            limit) are queued before the host reads the status words back.
//   algebra  union, intersection, complement on 64-bit words; complement clears the bits at and above n
//   rows     per-word popcount, exclusive scan, one wavefront per word emits (node, depth) at its ranks
//
// Depths: the reference keeps a depth map only for the ROOT of the expression; every pass that writes one claims nodes no
// other pass of the same expression claims (the two passes of `+x+` share a visited set), so one zero-filled int32[n] serves.
// An atom under a set operator has no depth map, which makes the reference read every depth as 0: its limit is ignored unless
// it is 0.  `N+x+M` keeps its own maps and honours its limits everywhere.
#include "mn_guard.hpp"
#include "mn_prim.hpp"

#include <rocprim/device/device_scan.hpp>

#include <climits>
#include <cstring>
#include <string>
#include <vector>

typedef unsigned long long sel_u64;

#define SEL_BLOCK 256
#define SEL_WAVES (SEL_BLOCK / 64)
#define SEL_LEVELS_PER_SYNC 16 // measured on a 20 000-node path
#define SEL_BOTTOM_UP_DIV 16   // auto: bottom-up when the frontier holds more than 1/16 of the direction's list entries
#define SEL_WHO "mn_graph_select"

// ───────────────────────── parser (host) ─────────────────────────
// graph_selector_parse.c restated: the same tokens, the same two back-tracking points, the same messages.

namespace {

enum SelTok { ST_IDENT, ST_PLUS, ST_AT, ST_COMMA, ST_NOT, ST_EOF };

struct SelLexer {
    const char *in, *pos;
    SelTok type;
    const char *start;
    int len;
    std::string err;
};

bool sel_alpha(char c) { return (c >= 'a' && c <= 'z') || (c >= 'A' && c <= 'Z'); } // the C locale's isalpha
bool sel_digit(char c) { return c >= '0' && c <= '9'; }
bool sel_name_char(char c) { return sel_alpha(c) || sel_digit(c) || c == '_' || c == '.' || c == '-'; }

void sel_blanks(SelLexer &lx) {
    while (*lx.pos == ' ' || *lx.pos == '\t')
        lx.pos++;
}

bool sel_next(SelLexer &lx) {
    sel_blanks(lx);
    const char c = *lx.pos;
    lx.start = lx.pos;
    if (c == '\0') {
        lx.type = ST_EOF;
        lx.len = 0;
        return true;
    }
    if (c == '+' || c == '@' || c == ',') {
        lx.type = c == '+' ? ST_PLUS : c == '@' ? ST_AT : ST_COMMA;
        lx.len = 1;
        lx.pos++;
        return true;
    }
    if (sel_alpha(c) || c == '_' || sel_digit(c)) {
        while (sel_name_char(*lx.pos))
            lx.pos++;
        lx.len = (int)(lx.pos - lx.start);
        lx.type = ST_IDENT;
        if (lx.len == 3 && !strncmp(lx.start, "not", 3)) { // a keyword unless the input ends or a comma follows (:106-121)
            sel_blanks(lx);
            const char nx = *lx.pos;
            if (!(nx == '\0' || nx == ',' || nx == ')'))
                lx.type = ST_NOT;
        }
        return true;
    }
    char buf[128];
    snprintf(buf, sizeof(buf), "graph_select: unexpected character '%c' at position %d", c, (int)(lx.pos - lx.in));
    lx.err = buf;
    return false;
}

bool sel_is_int(const SelLexer &lx) {
    if (lx.type != ST_IDENT || lx.len == 0)
        return false;
    for (int i = 0; i < lx.len; i++)
        if (!sel_digit(lx.start[i]))
            return false;
    return true;
}

// the reference's int overflows at ten digits and its behaviour there is undefined: saturate
int sel_to_int(const SelLexer &lx) {
    long long v = 0;
    for (int i = 0; i < lx.len; i++) {
        v = v * 10 + (lx.start[i] - '0');
        if (v > INT_MAX)
            return INT_MAX;
    }
    return (int)v;
}

struct SelSaved {
    const char *pos, *start;
    SelTok type;
    int len;
};
SelSaved sel_save(const SelLexer &lx) { return {lx.pos, lx.start, lx.type, lx.len}; }
void sel_restore(SelLexer &lx, const SelSaved &s) {
    lx.pos = s.pos;
    lx.start = s.start;
    lx.type = s.type;
    lx.len = s.len;
}

bool sel_atom(SelLexer &lx, std::vector<mn_select_op> &out) { // parse_atom (:217-374)
    bool at = false, pre = false, suf = false;
    int up = -1, down = -1;
    if (lx.type == ST_AT) {
        at = true;
        if (!sel_next(lx))
            return false;
    }
    if (lx.type == ST_PLUS) {
        pre = true;
        if (!sel_next(lx))
            return false;
    } else if (sel_is_int(lx)) { // INT "+" name, or a name made of digits
        const int v = sel_to_int(lx);
        const SelSaved s = sel_save(lx);
        if (!sel_next(lx))
            return false;
        if (lx.type == ST_PLUS) {
            up = v;
            pre = true;
            if (!sel_next(lx))
                return false;
        } else
            sel_restore(lx, s);
    }
    if (lx.type != ST_IDENT) {
        char buf[128];
        snprintf(buf, sizeof(buf), "graph_select: expected node name at position %d", (int)(lx.start - lx.in));
        lx.err = buf;
        return false;
    }
    const int name_off = (int)(lx.start - lx.in), name_len = lx.len;
    if (!sel_next(lx))
        return false;
    if (lx.type == ST_PLUS) { // the name's suffix only if an integer, the end or a comma follows (:287-314)
        const SelSaved s = sel_save(lx);
        if (!sel_next(lx))
            return false;
        if (sel_is_int(lx)) {
            suf = true;
            down = sel_to_int(lx);
            if (!sel_next(lx))
                return false;
        } else if (lx.type == ST_EOF || lx.type == ST_COMMA)
            suf = true;
        else
            sel_restore(lx, s);
    }
    mn_select_op op;
    op.node = -1;
    op.depth_up = op.depth_down = -1;
    op.name_off = name_off;
    op.name_len = name_len;
    if (at)
        op.op = MN_SEL_CLOSURE; // `@+x`, `@x+`: the modifiers are dropped (:319-330)
    else if (pre && suf) {
        op.op = MN_SEL_BOTH;
        op.depth_up = up;
        op.depth_down = down;
    } else if (pre) {
        op.op = MN_SEL_ANCESTORS;
        op.depth_up = up;
    } else if (suf) {
        op.op = MN_SEL_DESCENDANTS;
        op.depth_down = down;
    } else
        op.op = MN_SEL_NODE;
    out.push_back(op);
    return true;
}

void sel_push_operator(std::vector<mn_select_op> &out, int op) {
    mn_select_op o;
    o.op = op;
    o.node = -1;
    o.depth_up = o.depth_down = -1;
    o.name_off = o.name_len = 0;
    out.push_back(o);
}

bool sel_term(SelLexer &lx, std::vector<mn_select_op> &out) { // "not" atom | atom {"," atom} (:380-426)
    if (lx.type == ST_NOT) {
        if (!sel_next(lx) || !sel_atom(lx, out))
            return false;
        sel_push_operator(out, MN_SEL_COMPLEMENT);
        return true;
    }
    if (!sel_atom(lx, out))
        return false;
    while (lx.type == ST_COMMA) {
        if (!sel_next(lx) || !sel_atom(lx, out))
            return false;
        sel_push_operator(out, MN_SEL_INTERSECT);
    }
    return true;
}

bool sel_starts_term(SelTok t) { return t == ST_IDENT || t == ST_PLUS || t == ST_AT || t == ST_NOT; }

} // namespace

extern "C" int mn_select_parse(const char *expr, mn_select_op **prog, int *n_ops) try {
    if (prog)
        *prog = nullptr;
    if (n_ops)
        *n_ops = 0;
    if (!prog || !n_ops) {
        gset_err("mn_select_parse: bad arguments");
        return -1;
    }
    if (!expr || !*expr) {
        gset_err("graph_select: empty selector expression");
        return -1;
    }
    SelLexer lx;
    lx.in = lx.pos = lx.start = expr;
    lx.type = ST_EOF;
    lx.len = 0;
    std::vector<mn_select_op> out;
    bool ok = sel_next(lx) && sel_term(lx, out);
    while (ok && sel_starts_term(lx.type)) { // union by juxtaposition, left-associative (:435-461)
        ok = sel_term(lx, out);
        if (ok)
            sel_push_operator(out, MN_SEL_UNION);
    }
    if (!ok) {
        gset_err("%s", lx.err.c_str());
        return -1;
    }
    if (lx.type != ST_EOF) {
        gset_err("graph_select: unexpected token at position %d", (int)(lx.start - lx.in));
        return -1;
    }
    mn_select_op *p = (mn_select_op *)malloc(out.size() * sizeof(mn_select_op));
    if (!p) {
        gset_err("mn_select_parse: out of host memory");
        return -1;
    }
    memcpy(p, out.data(), out.size() * sizeof(mn_select_op));
    *prog = p;
    *n_ops = (int)out.size();
    return 0;
} MN_GUARD_END(gset_err, MN_NOTHING, -1)

// ───────────────────────── device ─────────────────────────

// status words of a reach, on the device; the host reads all of them back once per group of levels
enum { SS_CNT0 = 0, SS_LEVELS = 3, SS_BOTTOM_UP = 4, SS_WORDS = 5 };

struct SelWork {
    size_t words = 0;           // 64-bit words of an n-bit set
    DevBuf<sel_u64> sets;       // [sets][words]: the three frontiers, the closure's descendants, then the stack
    DevBuf<int> depth;          // [n]
    DevBuf<unsigned> wcnt, woff; // [words + 1] popcounts and their exclusive sums
    DevBuf<int> o_node, o_depth; // [n]
    DevBuf<sel_u64> status;     // [SS_WORDS]
    DevBuf<char> tmp;           // rocPRIM's
    std::vector<int> r_node, r_depth; // the rows of the last call
    bool rows_valid = false;
};

void sel_work_free(SelWork *w) { delete w; }

struct SelLevel {
    int n;
    unsigned words;
    const int *off, *tgt;   // the lists the traversal follows
    const int *ooff, *otgt; // the opposite lists (bottom-up)
    sel_u64 *visited;
    const sel_u64 *f_prev;
    sel_u64 *f_next, *f_clear;
    sel_u64 *status;
    int *depth; // null = not tracked
    int level;  // depth of the nodes this level discovers, >= 1
    int mode;   // 0 top-down, 1 bottom-up, 2 chosen from the frontier's entry count
    sel_u64 entries_dir; // list entries of the direction
    unsigned bu_div;
};

DEVI sel_u64 sel_wave_sum(sel_u64 v) {
    for (int s = 32; s > 0; s >>= 1)
        v += __shfl_xor(v, s, 64);
    return v;
}

// V |= seeds, F0 = seeds, F1 = 0, cnt[0] = the seeds' list entries (status[0..2] are zero on entry).  `seeds` null: the one node `seed`.
__global__ void __launch_bounds__(SEL_BLOCK) k_sel_seed(unsigned words, const int *off, sel_u64 *visited, const sel_u64 *seeds, int seed,
                                                        sel_u64 *f0, sel_u64 *f1, sel_u64 *status) {
    const unsigned w = blockIdx.x * SEL_WAVES + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (w >= words) // (whole wavefronts leave)
        return;
    const sel_u64 s = seeds ? seeds[w] : ((unsigned)(seed >> 6) == w ? (sel_u64)1 << (seed & 63) : 0);
    sel_u64 mine = 0;
    if ((s >> lane) & 1) {
        const int u = (int)(w * 64 + lane);
        mine = (sel_u64)(off[u + 1] - off[u]);
    }
    mine = sel_wave_sum(mine);
    if (lane == 0) {
        if (s)
            visited[w] |= s;
        f0[w] = s;
        f1[w] = 0;
        if (mine)
            atomicAdd(&status[SS_CNT0], mine);
    }
}

__global__ void __launch_bounds__(SEL_BLOCK) k_sel_level(SelLevel a) {
    __shared__ unsigned pre[SEL_WAVES][64];
    __shared__ int first[SEL_WAVES][64];
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const unsigned w = blockIdx.x * SEL_WAVES + wv;
    const int L = a.level;
    const sel_u64 prev = a.status[SS_CNT0 + (L - 1) % 3]; // list entries of the frontier: final since the launch before
    const bool bottom_up = a.mode == 1 || (a.mode == 2 && prev * a.bu_div > a.entries_dir);
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        a.status[SS_CNT0 + (L + 1) % 3] = 0; // nobody else touches this word during this launch
        if (prev) {
            a.status[SS_LEVELS] += 1;
            if (bottom_up)
                a.status[SS_BOTTOM_UP] += 1;
        }
    }
    if (prev == 0) // an empty frontier, or one without list entries: nothing can be discovered (the same in every workgroup)
        return;
    const bool live = w < a.words;
    if (live && lane == 0)
        a.f_clear[w] = 0;
    sel_u64 mine = 0;
    if (bottom_up) {
        if (!live)
            return;
        const sel_u64 vis = a.visited[w];
        const long long v = (long long)w * 64 + lane;
        int hit = 0;
        if (v < a.n && !((vis >> lane) & 1)) {
            const int e1 = a.ooff[v + 1];
            for (int e = a.ooff[v]; e < e1; e++) {
                const int u = a.otgt[e];
                if ((a.f_prev[u >> 6] >> (u & 63)) & 1) {
                    hit = 1;
                    break;
                }
            }
        }
        const sel_u64 b = __ballot(hit);
        if (hit) {
            if (a.depth)
                a.depth[v] = L;
            mine = (sel_u64)(a.off[v + 1] - a.off[v]);
        }
        if (lane == 0) {
            a.f_next[w] = b;
            if (b)
                a.visited[w] = vis | b;
        }
    } else {
        const sel_u64 word = live ? a.f_prev[w] : 0;
        const bool in_frontier = (word >> lane) & 1;
        int s = 0;
        unsigned d = 0;
        if (in_frontier) { // (bits at and above n are never set)
            const long long u = (long long)w * 64 + lane;
            s = a.off[u];
            d = (unsigned)(a.off[u + 1] - s);
        }
        unsigned incl = d;
        for (int k = 1; k < 64; k <<= 1) {
            const unsigned t = __shfl_up(incl, k, 64);
            if (lane >= k)
                incl += t;
        }
        pre[wv][lane] = incl - d;
        first[wv][lane] = s;
        const unsigned total = __shfl(incl, 63, 64);
        __syncthreads(); // (every thread of the workgroup arrives: nothing above returns in this branch)
        for (unsigned base = 0; base < total; base += 64) {
            const unsigned e = base + lane;
            if (e >= total)
                continue;
            int lo = 0, hi = 63; // the last node whose exclusive sum is <= e: the one entry e belongs to
            while (lo < hi) {
                const int mid = (lo + hi + 1) >> 1;
                if (pre[wv][mid] <= e)
                    lo = mid;
                else
                    hi = mid - 1;
            }
            const int v = a.tgt[first[wv][lo] + (int)(e - pre[wv][lo])];
            const sel_u64 bit = (sel_u64)1 << (v & 63);
            if (a.visited[v >> 6] & bit) // (bits are never cleared: a set bit read here, however stale, is set)
                continue;
            const sel_u64 old = atomicOr(&a.visited[v >> 6], bit);
            if (old & bit)
                continue;
            if (a.depth)
                a.depth[v] = L;
            atomicOr(&a.f_next[v >> 6], bit);
            mine += (sel_u64)(a.off[v + 1] - a.off[v]);
        }
    }
    mine = sel_wave_sum(mine);
    if (lane == 0 && mine)
        atomicAdd(&a.status[SS_CNT0 + L % 3], mine);
}

// op: MN_SEL_UNION / INTERSECT (dst = a op b) or COMPLEMENT (dst = ~a below n)
__global__ void __launch_bounds__(SEL_BLOCK) k_sel_algebra(int op, unsigned words, int n, sel_u64 *dst, const sel_u64 *x, const sel_u64 *y) {
    const unsigned w = blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= words)
        return;
    sel_u64 r;
    if (op == MN_SEL_UNION)
        r = x[w] | y[w];
    else if (op == MN_SEL_INTERSECT)
        r = x[w] & y[w];
    else {
        r = ~x[w];
        if (w == words - 1 && (n & 63))
            r &= ((sel_u64)1 << (n & 63)) - 1;
    }
    dst[w] = r;
}

__global__ void __launch_bounds__(SEL_BLOCK) k_sel_popcount(unsigned words, const sel_u64 *set, unsigned *wcnt) {
    const unsigned w = blockIdx.x * blockDim.x + threadIdx.x;
    if (w <= words) // one entry past the end, so that the exclusive sums end in the total
        wcnt[w] = w < words ? (unsigned)__popcll(set[w]) : 0u;
}

__global__ void __launch_bounds__(SEL_BLOCK) k_sel_emit(unsigned words, const sel_u64 *set, const unsigned *woff, const int *depth, int *o_node,
                                                        int *o_depth) {
    const unsigned w = blockIdx.x * SEL_WAVES + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (w >= words)
        return;
    const sel_u64 word = set[w];
    if (!((word >> lane) & 1))
        return;
    const unsigned r = woff[w] + (unsigned)__popcll(word & (((sel_u64)1 << lane) - 1));
    const int v = (int)(w * 64 + lane);
    o_node[r] = v;
    o_depth[r] = depth[v];
}

// ───────────────────────── host ─────────────────────────

namespace {

struct SelRun {
    mn_graph *g;
    SelWork *w;
    hipStream_t st;
    int mode, group;
    unsigned bu_div;
    int64_t levels = 0, launches = 0, syncs = 0, bottom_up = 0;
    double device_ms = 0;
    sel_u64 *set(size_t i) const { return w->sets.p + i * w->words; }
};

enum { SET_F0 = 0, SET_DESC = 3, SET_STACK = 4 };

unsigned sel_wave_grid(size_t words) { return (unsigned)((words + SEL_WAVES - 1) / SEL_WAVES); }

// the traversal from seed set `seeds` (null: the node `seed`) into `visited`; limit < 0 = none
int sel_reach(SelRun &r, sel_u64 *visited, const sel_u64 *seeds, int seed, bool forward, int limit, bool tracked) {
    mn_graph *g = r.g;
    SelWork *w = r.w;
    const unsigned words = (unsigned)w->words;
    const int *off = forward ? g->off_out : g->off_in, *tgt = forward ? g->tgt_out : g->tgt_in;
    GCHK(hipEventRecord(g->ev0, r.st));
    GCHK(hipMemsetAsync(w->status, 0, SS_WORDS * sizeof(sel_u64), r.st));
    hipLaunchKernelGGL(k_sel_seed, dim3(sel_wave_grid(words)), dim3(SEL_BLOCK), 0, r.st, words, off, visited, seeds, seed, r.set(SET_F0),
                       r.set(SET_F0 + 1), w->status);
    SelLevel a;
    a.n = g->n;
    a.words = words;
    a.off = off;
    a.tgt = tgt;
    a.ooff = forward ? g->off_in : g->off_out;
    a.otgt = forward ? g->tgt_in : g->tgt_out;
    a.visited = visited;
    a.status = w->status;
    a.depth = tracked ? w->depth.p : nullptr;
    a.mode = r.mode;
    a.entries_dir = (sel_u64)(forward ? g->e_out : g->e_in);
    a.bu_div = r.bu_div;
    const long long last = limit < 0 ? (long long)g->n : std::min<long long>(limit, g->n); // (a shortest path has fewer than n steps)
    sel_u64 h[SS_WORDS] = {0, 0, 0, 0, 0};
    long long L = 1;
    while (L <= last) {
        const long long G = std::min<long long>(r.group, last - L + 1);
        for (long long k = 0; k < G; k++, L++) {
            a.level = (int)L;
            a.f_prev = r.set(SET_F0 + (size_t)((L - 1) % 3));
            a.f_next = r.set(SET_F0 + (size_t)(L % 3));
            a.f_clear = r.set(SET_F0 + (size_t)((L + 1) % 3));
            hipLaunchKernelGGL(k_sel_level, dim3(sel_wave_grid(words)), dim3(SEL_BLOCK), 0, r.st, a);
        }
        r.launches += G;
        if (graph_mark(g))
            return -1;
        GCHK(hipMemcpyAsync(h, w->status, sizeof(h), hipMemcpyDeviceToHost, r.st)); // the group's one round trip
        if (graph_wait(g, &r.device_ms))
            return -1;
        r.syncs++;
        GCHK(hipEventRecord(g->ev0, r.st));
        if (h[SS_CNT0 + (L - 1) % 3] == 0) // the last level queued found nothing that has a list
            break;
    }
    r.levels += (int64_t)h[SS_LEVELS];
    r.bottom_up += (int64_t)h[SS_BOTTOM_UP];
    if (L == 1) // no level was queued: the seeding alone
        return graph_mark_wait(g, &r.device_ms);
    return 0;
}

int sel_env_int(const char *name, int dflt, int lo, int hi) {
    const char *e = getenv(name);
    if (!e || !*e)
        return dflt;
    char *end = nullptr;
    const long v = strtol(e, &end, 10);
    if (end == e || *end != '\0')
        return dflt;
    return (int)std::max<long>(lo, std::min<long>(hi, v));
}

} // namespace

extern "C" int64_t mn_graph_select(mn_graph *g, const mn_select_op *prog, int n_ops, mn_select_stats *stats) try {
    if (stats)
        memset(stats, 0, sizeof(*stats));
    if (!g) {
        gset_err("mn_graph_select: no graph");
        return -1;
    }
    GCHK(hipSetDevice(g->device));
    if (g->sel)
        g->sel->rows_valid = false;
    const int N = g->n;
    if (!prog || n_ops <= 0) {
        gset_err("mn_graph_select: an empty program");
        return -1;
    }
    if (g->e_out != g->e_in) {
        gset_err("mn_graph_select: the graph must hold out- and in-lists of the same edges (%lld out entries, %lld in entries)", g->e_out,
                 g->e_in);
        return -1;
    }
    // the program is checked whole before anything is launched: operands, stack discipline, node indices
    int sp = 0, max_sp = 0;
    for (int i = 0; i < n_ops; i++) {
        const mn_select_op &o = prog[i];
        if (o.op >= MN_SEL_NODE && o.op <= MN_SEL_CLOSURE) {
            if (o.node < 0 || o.node >= N) {
                gset_err("mn_graph_select: op %d names node %d, outside 0 .. %d", i, o.node, N - 1);
                return -1;
            }
            sp++;
        } else if (o.op == MN_SEL_UNION || o.op == MN_SEL_INTERSECT) {
            if (sp < 2) {
                gset_err("mn_graph_select: op %d has fewer than two operands", i);
                return -1;
            }
            sp--;
        } else if (o.op == MN_SEL_COMPLEMENT) {
            if (sp < 1) {
                gset_err("mn_graph_select: op %d has no operand", i);
                return -1;
            }
        } else {
            gset_err("mn_graph_select: op %d has unknown code %d", i, o.op);
            return -1;
        }
        max_sp = std::max(max_sp, sp);
    }
    if (sp != 1) {
        gset_err("mn_graph_select: the program leaves %d sets, not one", sp);
        return -1;
    }
    if (!g->sel)
        g->sel = new SelWork();
    SelWork *w = g->sel;
    w->r_node.clear();
    w->r_depth.clear();
    g->last_ms = 0;
    hipStream_t st = g->stream;
    const size_t words = ((size_t)N + 63) / 64;
    w->words = words;
    // the arrays sized by n alone: those a failed call left in place are found again by the next
    if (w->depth.fit(gset_err, SEL_WHO, (size_t)N) || w->o_node.fit(gset_err, SEL_WHO, (size_t)N) ||
        w->o_depth.fit(gset_err, SEL_WHO, (size_t)N) || w->wcnt.fit(gset_err, SEL_WHO, words + 1) ||
        w->woff.fit(gset_err, SEL_WHO, words + 1) || w->status.fit(gset_err, SEL_WHO, SS_WORDS)) {
        gset_err("mn_graph_select: out of device memory (N = %d)", N);
        return -1;
    }
    const size_t need_sets = SET_STACK + (size_t)max_sp;
    if (w->sets.fit(gset_err, SEL_WHO, need_sets * words)) {
        gset_err("mn_graph_select: out of device memory (%zu sets of %d bits)", need_sets, N);
        return -1;
    }
    SelRun r;
    r.g = g;
    r.w = w;
    r.st = st;
    r.group = sel_env_int("MN_SELECT_LEVELS_PER_SYNC", SEL_LEVELS_PER_SYNC, 1, 1 << 20);
    r.bu_div = (unsigned)sel_env_int("MN_SELECT_BOTTOM_UP_DIV", SEL_BOTTOM_UP_DIV, 1, 1 << 20);
    r.mode = 2;
    if (const char *e = getenv("MN_SELECT_BOTTOM_UP")) {
        if (!strcmp(e, "0"))
            r.mode = 0;
        else if (!strcmp(e, "1"))
            r.mode = 1;
        else if (*e && strcmp(e, "auto")) {
            gset_err("mn_graph_select: MN_SELECT_BOTTOM_UP must be 0, 1 or auto, not '%s'", e);
            return -1;
        }
    }
    GCHK(hipMemsetAsync(w->depth, 0, (size_t)N * sizeof(int), st));
    const bool root_is_atom = n_ops == 1; // the only operator-free program; the root's depth map is the only one kept
    const size_t set_bytes = words * sizeof(sel_u64);
    sp = 0;
    for (int i = 0; i < n_ops; i++) {
        const mn_select_op &o = prog[i];
        if (o.op >= MN_SEL_NODE && o.op <= MN_SEL_CLOSURE) {
            sel_u64 *V = r.set(SET_STACK + (size_t)sp++);
            GCHK(hipMemsetAsync(V, 0, set_bytes, st));
            // without a depth map the reference reads every depth as 0: a limit stops the traversal only if it is 0
            const int up = root_is_atom || o.op == MN_SEL_BOTH ? o.depth_up : (o.depth_up == 0 ? 0 : -1);
            const int down = root_is_atom || o.op == MN_SEL_BOTH ? o.depth_down : (o.depth_down == 0 ? 0 : -1);
            int rc = 0;
            switch (o.op) {
            case MN_SEL_NODE:
                rc = sel_reach(r, V, nullptr, o.node, true, 0, false);
                break;
            case MN_SEL_ANCESTORS:
                rc = sel_reach(r, V, nullptr, o.node, false, up, root_is_atom);
                break;
            case MN_SEL_DESCENDANTS:
                rc = sel_reach(r, V, nullptr, o.node, true, down, root_is_atom);
                break;
            case MN_SEL_BOTH: // the descendant pass runs under the ancestors' visited set (:347-357)
                rc = sel_reach(r, V, nullptr, o.node, false, up, root_is_atom);
                if (rc == 0)
                    rc = sel_reach(r, V, nullptr, o.node, true, down, root_is_atom);
                break;
            default: { // MN_SEL_CLOSURE: every descendant, then every ancestor of that whole set (:377-411)
                sel_u64 *D = r.set(SET_DESC);
                GCHK(hipMemsetAsync(D, 0, set_bytes, st));
                rc = sel_reach(r, D, nullptr, o.node, true, -1, false);
                if (rc == 0)
                    rc = sel_reach(r, V, D, -1, false, -1, root_is_atom);
                break;
            }
            }
            if (rc != 0)
                return -1;
        } else if (o.op == MN_SEL_COMPLEMENT) {
            sel_u64 *x = r.set(SET_STACK + (size_t)sp - 1);
            hipLaunchKernelGGL(k_sel_algebra, dim3((unsigned)((words + SEL_BLOCK - 1) / SEL_BLOCK)), dim3(SEL_BLOCK), 0, st, o.op,
                               (unsigned)words, N, x, x, x);
        } else {
            sel_u64 *x = r.set(SET_STACK + (size_t)sp - 2), *y = r.set(SET_STACK + (size_t)sp - 1);
            hipLaunchKernelGGL(k_sel_algebra, dim3((unsigned)((words + SEL_BLOCK - 1) / SEL_BLOCK)), dim3(SEL_BLOCK), 0, st, o.op,
                               (unsigned)words, N, x, x, y);
            sp--;
        }
    }
    // rows: popcount per word, exclusive sums, one wavefront per word writes its nodes at their ranks
    const sel_u64 *result = r.set(SET_STACK);
    GCHK(hipEventRecord(g->ev0, st));
    hipLaunchKernelGGL(k_sel_popcount, dim3((unsigned)((words + 1 + SEL_BLOCK - 1) / SEL_BLOCK)), dim3(SEL_BLOCK), 0, st, (unsigned)words,
                       result, w->wcnt);
    if (prim_run(SEL_WHO, "rocprim::exclusive_scan", w->tmp, st, [&](void *tmp, size_t &bytes) {
            return rocprim::exclusive_scan(tmp, bytes, w->wcnt.p, w->woff.p, 0u, words + 1, rocprim::plus<unsigned>(), st);
        }))
        return -1;
    hipLaunchKernelGGL(k_sel_emit, dim3(sel_wave_grid(words)), dim3(SEL_BLOCK), 0, st, (unsigned)words, result, w->woff, w->depth, w->o_node,
                       w->o_depth);
    if (graph_mark(g))
        return -1;
    unsigned total = 0;
    GCHK(hipMemcpyAsync(&total, w->woff.p + words, sizeof(unsigned), hipMemcpyDeviceToHost, st));
    if (graph_wait(g, &r.device_ms))
        return -1;
    if (total > (unsigned)N) {
        gset_err("mn_graph_select: %u rows from %d nodes", total, N);
        return -1;
    }
    w->r_node.resize(total);
    w->r_depth.resize(total);
    if (total) {
        GCHK(hipMemcpyAsync(w->r_node.data(), w->o_node, (size_t)total * sizeof(int), hipMemcpyDeviceToHost, st));
        GCHK(hipMemcpyAsync(w->r_depth.data(), w->o_depth, (size_t)total * sizeof(int), hipMemcpyDeviceToHost, st));
        GCHK(hipStreamSynchronize(st));
    }
    g->last_ms = r.device_ms;
    if (stats) {
        stats->rows = total;
        stats->levels = r.levels;
        stats->launches = r.launches;
        stats->syncs = r.syncs;
        stats->bottom_up_levels = r.bottom_up;
        stats->device_ms = r.device_ms;
    }
    w->rows_valid = true;
    return (int64_t)total;
} MN_GUARD_END(gset_err, MN_NOTHING, -1)

extern "C" int mn_graph_select_rows(mn_graph *g, int *node, int *depth) try {
    const SelWork *w = g ? g->sel : nullptr;
    if (!w || !w->rows_valid) {
        gset_err("mn_graph_select_rows: no rows (the last mn_graph_select on this graph failed, or there was none)");
        return -1;
    }
    const size_t bytes = w->r_node.size() * sizeof(int);
    if (bytes) {
        if (node)
            memcpy(node, w->r_node.data(), bytes);
        if (depth)
            memcpy(depth, w->r_depth.data(), bytes);
    }
    return 0;
} MN_GUARD_END(gset_err, MN_NOTHING, -1)
