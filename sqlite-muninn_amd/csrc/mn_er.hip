// mn_er.hip — the middle stages of the reference's entity resolution (src/llama_er.c) on the device, gfx950:
//   mn_er_jaro_winkler   jaro_winkler (src/string_sim.c:11-96) over byte strings, to the f64 bit
//   mn_er_candidates     the candidate loop and its de-duplication (src/llama_er.c:237-284) without the quadratic scan
//   mn_er_score          the type guard and the scoring cascade (src/llama_er.c:295-332)
//   mn_hnsw_er_edges     blocking (mn_hnsw_search_batch_dev or mn_hnsw_knn_graph_dev) + the two stages above on the index's
//                        device and stream: names go up, match edges come down
//
// Jaro-Winkler.  Everything up to the last two lines of the reference is integer work and exact in any order that keeps the
// reference's greedy rule: s1 is walked left to right and every byte takes the FIRST unmatched equal byte of s2 inside its window.
// The f64 tail is written as the reference writes it; the library is built with -ffp-contract=off, f64 division is correctly
// rounded on gfx950, and no fma is called, so the bits are the host's.
//   Short path (both names <= 64 bytes): one pair per lane.  The two "matched" sets are two 64-bit masks in registers; the pair's
//   bytes are staged in LDS (a per-lane array indexed at run time would live in scratch memory), one row of ER_ROW bytes per
//   lane — 17 dwords, an odd stride, so lanes at the same position fall into different banks.  A wavefront stages its 64 pairs
//   together: 64 lanes copy one name's bytes side by side.
//   Long path (either name longer): one wavefront per pair, after the short pairs of the same 64 are done.  Both names are staged in
//   LDS; the walk over s1 stays sequential; the window is scanned 64 bytes at a time, ascending, with a ballot and a find-first;
//   the matched bits live in LDS (2 x 4096 bits).  Transpositions: the matched bytes of either name are compacted in place (rank =
//   matched bytes before it), then compared rank by rank by the whole wavefront.
// One launch serves both: a block is one wavefront and owns 64 consecutive pairs.
//
// Candidates.  The reference appends an unordered pair (lo, hi) when it first meets it over (entity ascending, list position
// ascending) and afterwards only lowers its distance.  With every id at most once in a list (a search's answer), a pair appears at
// most twice, once in either end's list, so an entry i -> j decides alone: j > i is the first appearance (kept; distance lowered
// by that of j -> i if j's filtered list holds i); j < i is a first appearance only if j's filtered list does not hold i.  The keep
// flags go through rocPRIM's exclusive scan and the kept entries are written in entry order: the reference's order.
#include "mn_index_int.hpp"
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#include <cmath>

#define ER_ROW 68        /* bytes of LDS per staged short name: 64 + 4, 17 dwords */
#define ER_MAX_NAME 4096 /* longest name the long path stages */
#define ER_WORDS (ER_MAX_NAME / 64)
#define DEVI_ER __device__ __forceinline__

// LDS of one wavefront: the short path's 2 x 64 rows and the long path's two names never live at the same time
struct ErLds {
    union {
        unsigned char rows[2][64 * ER_ROW];
        unsigned char name[2][ER_MAX_NAME];
    };
    unsigned long long m[2][ER_WORDS];
};

DEVI_ER unsigned char er_lower(unsigned char c) { return (c >= 'A' && c <= 'Z') ? (unsigned char)(c + 32) : c; } // tolower, C locale

// string_sim.c:80-95: the f64 tail in the reference's order
DEVI_ER double er_jw_tail(int matches, int transpositions, int len1, int len2, int prefix) {
    const double m = (double)matches;
    const double jaro = (m / len1 + m / len2 + (m - transpositions / 2.0) / matches) / 3.0;
    return jaro + prefix * 0.1 * (1.0 - jaro);
}

DEVI_ER int er_match_dist(int len1, int len2) { // :22-24
    const int md = (len1 > len2 ? len1 : len2) / 2 - 1;
    return md < 0 ? 0 : md;
}

// One pair per lane, names staged (and, LOWER, already lowered) in the lane's rows; 1 <= len <= 64, names not equal.
DEVI_ER double er_jw_short(const unsigned char *s1, const unsigned char *s2, int len1, int len2) {
    const int md = er_match_dist(len1, len2);
    unsigned long long m1 = 0, m2 = 0;
    int matches = 0;
    for (int i = 0; i < len1; i++) { // :38-53
        const int lo = i - md < 0 ? 0 : i - md;
        const int hi = i + md + 1 > len2 ? len2 : i + md + 1;
        const unsigned char c = s1[i];
        for (int j = lo; j < hi; j++) {
            if (((m2 >> j) & 1ull) || s2[j] != c)
                continue;
            m1 |= 1ull << i;
            m2 |= 1ull << j;
            matches++;
            break;
        }
    }
    if (matches == 0)
        return 0.0;
    int t = 0; // :64-73: the r-th matched byte of s1 against the r-th matched byte of s2
    while (m1) {
        const int i = __builtin_ctzll(m1), j = __builtin_ctzll(m2);
        m1 &= m1 - 1;
        m2 &= m2 - 1;
        t += s1[i] != s2[j];
    }
    int prefix = 0; // :84-93
    const int mp = len1 < len2 ? (len1 < 4 ? len1 : 4) : (len2 < 4 ? len2 : 4);
    while (prefix < mp && s1[prefix] == s2[prefix])
        prefix++;
    return er_jw_tail(matches, t, len1, len2, prefix);
}

// One wavefront per pair, names staged in L.name; every lane returns the same value.  1 <= len <= ER_MAX_NAME, names not equal.
DEVI_ER double er_jw_long(ErLds &L, int len1, int len2, int lane) {
    unsigned char *s1 = L.name[0], *s2 = L.name[1];
    const int md = er_match_dist(len1, len2);
    L.m[0][lane] = 0; // ER_WORDS == 64 == lanes
    L.m[1][lane] = 0;
    __syncthreads();
    int prefix = 0;
    const int mp = len1 < len2 ? (len1 < 4 ? len1 : 4) : (len2 < 4 ? len2 : 4);
    while (prefix < mp && s1[prefix] == s2[prefix])
        prefix++;
    int matches = 0;
    for (int i = 0; i < len1; i++) {
        const int lo = i - md < 0 ? 0 : i - md;
        const int hi = i + md + 1 > len2 ? len2 : i + md + 1;
        const unsigned char c = s1[i];
        for (int base = lo & ~63; base < hi; base += 64) {
            const int j = base + lane;
            // every lane writes the same word below and reads it back here: its own program order is all that is needed
            const unsigned long long w = L.m[1][base >> 6];
            const bool ok = j >= lo && j < hi && s2[j] == c && !((w >> lane) & 1ull);
            const unsigned long long b = __ballot(ok);
            if (b) {
                const int f = __builtin_ctzll(b);
                L.m[1][base >> 6] = w | (1ull << f);
                L.m[0][i >> 6] = L.m[0][i >> 6] | (1ull << (i & 63));
                matches++;
                break;
            }
        }
    }
    if (matches == 0)
        return 0.0;
    __syncthreads();
    // compaction in place: the byte at position p moves to its rank <= p; a word's bytes are read before any of them is written
    for (int side = 0; side < 2; side++) {
        const int len = side ? len2 : len1;
        unsigned char *s = side ? s2 : s1;
        int rank0 = 0;
        for (int w = 0; w * 64 < len; w++) {
            const unsigned long long bits = L.m[side][w];
            const unsigned char c = s[w * 64 + lane]; // (inside the 4096 staged bytes whatever len is)
            __syncthreads();
            if ((bits >> lane) & 1ull)
                s[rank0 + __builtin_popcountll(bits & ((1ull << lane) - 1ull))] = c;
            rank0 += __builtin_popcountll(bits);
            __syncthreads();
        }
    }
    int t = 0;
    for (int r = lane; r < matches; r += 64)
        t += s1[r] != s2[r];
    for (int o = 32; o; o >>= 1)
        t += __shfl_xor(t, o);
    return er_jw_tail(matches, t, len1, len2, prefix);
}

// What a wavefront does with its 64 pairs.  Lane's pair: names at bytes + oa / ob of la / lb bytes; act = the lane has a pair.
// SCORE: the cascade's tiers are decided on the way (tier 2: names equal byte for byte, 1: equal after lowering, 0: neither) and
// Jaro-Winkler is taken on the lowered names (src/llama_er.c:315-321); otherwise the names are compared as they are and an equal
// pair answers 1.0 (string_sim.c:19).  path[0] / path[1] count the pairs that went through the short / long matching loop.
template <bool SCORE>
DEVI_ER double er_wave_pairs(ErLds &L, const unsigned char *bytes, long long oa, int la, long long ob, int lb, bool act, int lane,
                             int &tier, unsigned long long *path) {
    tier = 0;
    double jw = 0.0;
    const bool is_long = act && (la > 64 || lb > 64);
    const bool is_short = act && !is_long;
    // ---- short pairs: staged together, one row per lane and name ----
    __syncthreads();
    for (int p = 0; p < 64; p++) {
        const long long poa = __shfl(oa, p), pob = __shfl(ob, p);
        const int pla = __shfl(is_short ? la : 0, p), plb = __shfl(is_short ? lb : 0, p);
        if (lane < pla)
            L.rows[0][p * ER_ROW + lane] = bytes[poa + lane];
        if (lane < plb)
            L.rows[1][p * ER_ROW + lane] = bytes[pob + lane];
    }
    __syncthreads();
    bool need = false; // the matching loop has to run
    if (is_short) {
        unsigned char *s1 = L.rows[0] + lane * ER_ROW, *s2 = L.rows[1] + lane * ER_ROW;
        bool eq = la == lb;
        for (int i = 0; eq && i < la; i++)
            eq = s1[i] == s2[i];
        if (eq) {
            tier = 2;
            jw = 1.0; // :15-16, :19-20
        } else if (SCORE) {
            for (int i = 0; i < la; i++)
                s1[i] = er_lower(s1[i]);
            for (int i = 0; i < lb; i++)
                s2[i] = er_lower(s2[i]);
            bool eql = la == lb;
            for (int i = 0; eql && i < la; i++)
                eql = s1[i] == s2[i];
            if (eql)
                tier = 1;
            need = !eql;
        } else {
            need = true;
        }
        if (need && (la == 0 || lb == 0)) { // :17-18
            need = false;
            jw = 0.0;
        }
        if (need)
            jw = er_jw_short(s1, s2, la, lb);
    }
    unsigned long long n_short = __ballot(need);
    // ---- long pairs: the wavefront takes them one after the other ----
    unsigned long long todo = __ballot(is_long);
    int n_long = 0;
    while (todo) {
        const int p = __builtin_ctzll(todo);
        todo &= todo - 1;
        const long long poa = __shfl(oa, p), pob = __shfl(ob, p);
        const int pla = __shfl(la, p), plb = __shfl(lb, p);
        __syncthreads();
        bool diff = false, diffl = false;
        // staged up to the longer name rounded up to 64: the window scan and the compaction read whole 64-byte words below a
        // name's end and nothing past them; past a name's end inside that range: zeros
        const int stage = ((pla > plb ? pla : plb) + 63) & ~63;
        for (int i = lane; i < stage; i += 64) {
            const unsigned char a = i < pla ? bytes[poa + i] : 0, b = i < plb ? bytes[pob + i] : 0;
            diff |= a != b;
            diffl |= er_lower(a) != er_lower(b);
            L.name[0][i] = SCORE ? er_lower(a) : a;
            L.name[1][i] = SCORE ? er_lower(b) : b;
        }
        const bool eq = pla == plb && !__any(diff), eql = pla == plb && !__any(diffl);
        int ptier = 0;
        double pjw = 0.0;
        if (eq) {
            ptier = 2;
            pjw = 1.0;
        } else if (SCORE && eql) {
            ptier = 1;
        } else if (pla == 0 || plb == 0) {
            pjw = 0.0;
        } else {
            __syncthreads();
            pjw = er_jw_long(L, pla, plb, lane);
            n_long++;
        }
        if (lane == p) {
            tier = ptier;
            jw = pjw;
        }
    }
    if (path && lane == 0) {
        if (n_short)
            atomicAdd(path + 0, (unsigned long long)__builtin_popcountll(n_short));
        if (n_long)
            atomicAdd(path + 1, (unsigned long long)n_long);
    }
    return jw;
}

__global__ void __launch_bounds__(64)
    k_er_jw(const unsigned char *bytes, const long long *off, const int *a, const int *b, long long n_pairs, double *out,
            unsigned long long *path) {
    __shared__ ErLds L;
    const int lane = threadIdx.x;
    const long long p = (long long)blockIdx.x * 64 + lane;
    const bool act = p < n_pairs;
    long long oa = 0, ob = 0;
    int la = 0, lb = 0;
    if (act) {
        oa = off[a[p]];
        la = (int)(off[a[p] + 1] - oa);
        ob = off[b[p]];
        lb = (int)(off[b[p] + 1] - ob);
    }
    int tier;
    const double jw = er_wave_pairs<false>(L, bytes, oa, la, ob, lb, act, lane, tier, path);
    if (act)
        out[p] = jw;
}

// ───────────────────────── candidate pairs from neighbour lists (src/llama_er.c:237-284) ─────────────────────────

// row_of (or null: i): the row of nbr_ids / nbr_dists / counts that holds entity i's list; < 0: the entity has no vector (:240-243)
DEVI_ER int er_row(const int *row_of, int i) { return row_of ? row_of[i] : i; }
DEVI_ER int er_count(const int *counts, int row, int kk) {
    if (row < 0)
        return 0;
    const int c = counts[row];
    return c < 0 ? 0 : (c > kk ? kk : c);
}

// jmap[i][p] = the entity the p-th entry of i's list names if the entry passes the three tests (:253-258), else -1
__global__ void k_er_resolve(const long long *ent_ids, const int *row_of, const long long *nbr_ids, const float *nbr_dists,
                             const int *counts, int n, int kk, double thr, const long long *sorted_ids, const int *sorted_idx,
                             int *jmap) {
    const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= (long long)n * kk)
        return;
    const int i = (int)(e / kk), p = (int)(e % kk);
    const int row = er_row(row_of, i);
    int j = -1;
    if (p < er_count(counts, row, kk)) {
        const long long id = nbr_ids[(size_t)row * kk + p];
        const double d = (double)nbr_dists[(size_t)row * kk + p];
        if (id != ent_ids[i] && !(d > thr)) {
            int lo = 0, hi = n; // first sorted id >= id
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (sorted_ids[mid] < id)
                    lo = mid + 1;
                else
                    hi = mid;
            }
            if (lo < n && sorted_ids[lo] == id)
                j = sorted_idx[lo];
        }
    }
    jmap[e] = j;
}

__global__ void k_er_decide(const int *row_of, const float *nbr_dists, const int *jmap, int n, int kk, int *keep, double *dmin) {
    const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= (long long)n * kk)
        return;
    const int i = (int)(e / kk), p = (int)(e % kk);
    const int j = jmap[e];
    int k = 0;
    if (j >= 0) {
        const int *jr = jmap + (size_t)j * kk;
        int q = -1;
        for (int t = 0; t < kk; t++)
            if (jr[t] == i) {
                q = t;
                break;
            }
        double d = (double)nbr_dists[(size_t)er_row(row_of, i) * kk + p];
        if (j > i) {
            if (q >= 0) { // :268-269: the later appearance only lowers the distance
                const double d2 = (double)nbr_dists[(size_t)er_row(row_of, j) * kk + q];
                if (d2 < d)
                    d = d2;
            }
            k = 1;
        } else {
            k = q < 0; // (j == i cannot be: the entity's own id is filtered and ids are unique)
        }
        dmin[e] = d;
    }
    keep[e] = k;
}

__global__ void k_er_emit_pairs(const int *jmap, const int *keep, const int *pos, const double *dmin, int n, int kk, int *r1, int *r2,
                                double *dist) {
    const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= (long long)n * kk || !keep[e])
        return;
    const int i = (int)(e / kk), j = jmap[e], o = pos[e];
    r1[o] = i < j ? i : j; // :261-262
    r2[o] = i < j ? j : i;
    dist[o] = dmin[e];
}

// ───────────────────────── type guard + scoring cascade (src/llama_er.c:295-332) ─────────────────────────

__global__ void __launch_bounds__(64)
    k_er_score(const int *r1, const int *r2, const double *dist, long long n_cand, const unsigned char *bytes, const long long *off,
               const int *source_id, int guard, double jw_weight, double match_threshold, int *keep, double *score,
               unsigned long long *path) {
    __shared__ ErLds L;
    const int lane = threadIdx.x;
    const long long c = (long long)blockIdx.x * 64 + lane;
    bool act = c < n_cand;
    long long oa = 0, ob = 0;
    int la = 0, lb = 0;
    if (act) {
        const int i = r1[c], j = r2[c];
        const int si = source_id ? source_id[i] : 0, sj = source_id ? source_id[j] : 0; // 0: the empty source, never blocks
        if (guard == MN_ER_GUARD_SAME_SOURCE && si && sj && si == sj) // :303-305
            act = false;
        if (guard == MN_ER_GUARD_DIFF_TYPE && si && sj && si != sj) // :306-308
            act = false;
        oa = off[i];
        la = (int)(off[i + 1] - oa);
        ob = off[j];
        lb = (int)(off[j + 1] - ob);
    }
    int tier;
    const double jw = er_wave_pairs<true>(L, bytes, oa, la, ob, lb, act, lane, tier, path);
    if (c < n_cand) {
        int k = 0;
        if (act) {
            const double cosine_sim = 1.0 - dist[c]; // :311
            const double s = tier == 2 ? 1.0 : tier == 1 ? 0.9 : jw_weight * jw + (1.0 - jw_weight) * cosine_sim; // :315-322
            k = s >= match_threshold; // :324
            score[c] = s;
        }
        keep[c] = k;
    }
}

__global__ void k_er_emit_edges(const int *r1, const int *r2, const int *keep, const int *pos, const double *score, long long n_cand,
                                mn_er_edge *edges) {
    const long long c = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= n_cand || !keep[c])
        return;
    mn_er_edge e;
    e.r1 = r1[c];
    e.r2 = r2[c];
    e.weight = score[c];
    edges[pos[c]] = e;
}

// ───────────────────────── blocking helpers of mn_hnsw_er_edges ─────────────────────────

// queries of the reference's search: the stored vector of every entity that has one (:239-248)
__global__ void k_er_gather(const float *vectors, int ld, int dim, const int *slot, int n, float *q) {
    const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= (long long)n * dim)
        return;
    const int i = (int)(e / dim), c = (int)(e % dim);
    const int s = slot[i];
    q[e] = vectors[(size_t)s * ld + c];
}

// the candidate rule needs every rowid once: *dup = 1 where the sorted ids hold one twice
__global__ void k_er_dup(const long long *sorted_ids, int n, int *dup) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i + 1 < n && sorted_ids[i] == sorted_ids[i + 1])
        *dup = 1;
}

__global__ void k_er_iota(int *v, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n)
        v[i] = i;
}

// ───────────────────────── host side ─────────────────────────

#define ER_GRID(n, b) dim3((unsigned)(((long long)(n) + (b) - 1) / (b)))

// keep[0..n) -> pos[0..n) (exclusive scan) and the number kept; synchronises the stream
static int er_scan(DevArena &A, hipStream_t st, const int *keep, int *pos, long long n, long long *total) {
    size_t bytes = 0;
    HIPCHK(rocprim::exclusive_scan(nullptr, bytes, keep, pos, 0, (size_t)n, rocprim::plus<int>(), st));
    void *tmp = A.alloc<unsigned char>(bytes ? bytes : 16);
    if (!tmp) {
        set_err("mn_er: out of device memory");
        return -1;
    }
    HIPCHK(rocprim::exclusive_scan(tmp, bytes, keep, pos, 0, (size_t)n, rocprim::plus<int>(), st));
    int last[2] = {0, 0};
    HIPCHK(hipMemcpyAsync(&last[0], keep + n - 1, sizeof(int), hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(&last[1], pos + n - 1, sizeof(int), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    *total = (long long)last[0] + last[1];
    return 0;
}

// Device arrays in, pairs out in d_r1 / d_r2 / d_dist (each n * kk); returns the pair count or -1.  Synchronises.
static long long er_candidates_dev(DevArena &A, hipStream_t st, int n, int kk, const long long *d_ent, const int *d_row_of,
                                   const long long *d_nids, const float *d_nd, const int *d_counts, double thr, int *d_r1, int *d_r2,
                                   double *d_dist) {
    if (n == 0)
        return 0;
    const long long ne = (long long)n * kk;
    long long *d_sid = A.alloc<long long>(n);
    int *d_idx = A.alloc<int>(n), *d_sidx = A.alloc<int>(n), *d_jmap = A.alloc<int>(ne), *d_keep = A.alloc<int>(ne), *d_pos = A.alloc<int>(ne);
    double *d_dmin = A.alloc<double>(ne);
    int *d_dup = A.alloc<int>(1);
    size_t sb = 0;
    HIPCHK(rocprim::radix_sort_pairs(nullptr, sb, d_ent, d_sid, d_idx, d_sidx, (size_t)n, 0, 64, st));
    void *tmp = A.alloc<unsigned char>(sb ? sb : 16);
    if (!d_sid || !d_idx || !d_sidx || !d_jmap || !d_keep || !d_pos || !d_dmin || !d_dup || !tmp) {
        set_err("mn_er_candidates: out of device memory");
        return -1;
    }
    hipLaunchKernelGGL(k_er_iota, ER_GRID(n, 256), dim3(256), 0, st, d_idx, n);
    HIPCHK(rocprim::radix_sort_pairs(tmp, sb, d_ent, d_sid, d_idx, d_sidx, (size_t)n, 0, 64, st));
    int dup = 0;
    HIPCHK(hipMemsetAsync(d_dup, 0, sizeof(int), st));
    hipLaunchKernelGGL(k_er_dup, ER_GRID(n, 256), dim3(256), 0, st, d_sid, n, d_dup);
    HIPCHK(hipMemcpyAsync(&dup, d_dup, sizeof(int), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (dup) {
        set_err("mn_er_candidates: ent_ids names an id twice");
        return -1;
    }
    hipLaunchKernelGGL(k_er_resolve, ER_GRID(ne, 256), dim3(256), 0, st, d_ent, d_row_of, d_nids, d_nd, d_counts, n, kk, thr, d_sid, d_sidx,
                       d_jmap);
    hipLaunchKernelGGL(k_er_decide, ER_GRID(ne, 256), dim3(256), 0, st, d_row_of, d_nd, d_jmap, n, kk, d_keep, d_dmin);
    long long total = 0;
    if (er_scan(A, st, d_keep, d_pos, ne, &total))
        return -1;
    hipLaunchKernelGGL(k_er_emit_pairs, ER_GRID(ne, 256), dim3(256), 0, st, d_jmap, d_keep, d_pos, d_dmin, n, kk, d_r1, d_r2, d_dist);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(st));
    return total;
}

// Device arrays in, edges out in d_edges (n_cand); d_path: 2 counters, added to.  Returns the edge count or -1.  Synchronises.
static long long er_score_dev(DevArena &A, hipStream_t st, long long n_cand, const int *d_r1, const int *d_r2, const double *d_dist,
                              const unsigned char *d_bytes, const long long *d_off, const int *d_src, int guard, double jw_weight,
                              double match_threshold, mn_er_edge *d_edges, unsigned long long *d_path) {
    if (n_cand == 0)
        return 0;
    int *d_keep = A.alloc<int>(n_cand), *d_pos = A.alloc<int>(n_cand);
    double *d_score = A.alloc<double>(n_cand);
    if (!d_keep || !d_pos || !d_score) {
        set_err("mn_er_score: out of device memory");
        return -1;
    }
    hipLaunchKernelGGL(k_er_score, ER_GRID(n_cand, 64), dim3(64), 0, st, d_r1, d_r2, d_dist, n_cand, d_bytes, d_off, d_src, guard, jw_weight,
                       match_threshold, d_keep, d_score, d_path);
    long long total = 0;
    if (er_scan(A, st, d_keep, d_pos, n_cand, &total))
        return -1;
    hipLaunchKernelGGL(k_er_emit_edges, ER_GRID(n_cand, 256), dim3(256), 0, st, d_r1, d_r2, d_keep, d_pos, d_score, n_cand, d_edges);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(st));
    return total;
}

// ---- argument checks, all before any launch ----
static int er_check_names(const char *fn, const unsigned char *bytes, const int64_t *off, int64_t n_str) {
    if (n_str < 0 || !off || n_str >= (1ll << 31)) {
        set_err("%s: bad name table (n = %lld)", fn, (long long)n_str);
        return -1;
    }
    if (off[0] < 0) {
        set_err("%s: name offsets must start at or after 0 (got %lld)", fn, (long long)off[0]);
        return -1;
    }
    for (int64_t i = 0; i < n_str; i++) {
        if (off[i + 1] < off[i]) {
            set_err("%s: name offsets are not monotone at name %lld", fn, (long long)i);
            return -1;
        }
        if (off[i + 1] - off[i] > ER_MAX_NAME) {
            set_err("%s: name %lld is %lld bytes long, more than the %d this library stages", fn, (long long)i,
                    (long long)(off[i + 1] - off[i]), ER_MAX_NAME);
            return -1;
        }
    }
    if (off[n_str] > off[0] && !bytes) {
        set_err("%s: names without bytes", fn);
        return -1;
    }
    return 0;
}

static int er_check_device(const char *fn, int device) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) {
        set_err("%s: HIP device %d not available (no CPU fallback)", fn, device);
        return -1;
    }
    HIPCHK(hipSetDevice(device));
    return 0;
}

template <typename T> static T *er_upload(DevArena &A, hipStream_t st, const T *h, size_t n) {
    T *d = A.alloc<T>(n);
    if (d && n && hipMemcpyAsync(d, h, n * sizeof(T), hipMemcpyHostToDevice, st) != hipSuccess)
        return nullptr;
    return d;
}

// the arena arrives as bytes [0, off[n_str]); the bytes before off[0] are never read
extern "C" int mn_er_jaro_winkler(int64_t n_pairs, const unsigned char *bytes, const int64_t *off, int64_t n_str, const int *a,
                                  const int *b, int device, double *out) try {
    if (n_pairs < 0 || (n_pairs && (!a || !b || !out))) {
        set_err("mn_er_jaro_winkler: bad arguments");
        return -1;
    }
    if (er_check_names("mn_er_jaro_winkler", bytes, off, n_str))
        return -1;
    for (int64_t p = 0; p < n_pairs; p++)
        if (a[p] < 0 || a[p] >= n_str || b[p] < 0 || b[p] >= n_str) {
            set_err("mn_er_jaro_winkler: pair %lld names a string outside [0, %lld)", (long long)p, (long long)n_str);
            return -1;
        }
    if (n_pairs == 0)
        return 0;
    if (er_check_device("mn_er_jaro_winkler", device))
        return -1;
    DevArena A;
    unsigned char *d_bytes = er_upload(A, nullptr, bytes, (size_t)off[n_str]);
    long long *d_off = er_upload(A, nullptr, (const long long *)off, (size_t)n_str + 1);
    int *d_a = er_upload(A, nullptr, a, (size_t)n_pairs), *d_b = er_upload(A, nullptr, b, (size_t)n_pairs);
    double *d_out = A.alloc<double>((size_t)n_pairs);
    if (!d_bytes || !d_off || !d_a || !d_b || !d_out) {
        set_err("mn_er_jaro_winkler: out of device memory");
        return -1;
    }
    hipLaunchKernelGGL(k_er_jw, ER_GRID(n_pairs, 64), dim3(64), 0, nullptr, d_bytes, d_off, d_a, d_b, (long long)n_pairs, d_out,
                       (unsigned long long *)nullptr);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpy(out, d_out, (size_t)n_pairs * sizeof(double), hipMemcpyDeviceToHost));
    return 0;
} MN_GUARD_END(set_err, MN_NOTHING, -1)

extern "C" int64_t mn_er_candidates(int n, int kk, const int64_t *ent_ids, const int64_t *nbr_ids, const float *nbr_dists,
                                    const int *counts, double dist_threshold, int device, int *r1, int *r2, double *dist) try {
    if (n < 0 || (n && (!ent_ids || !nbr_ids || !nbr_dists || !counts || !r1 || !r2 || !dist))) {
        set_err("mn_er_candidates: bad arguments");
        return -1;
    }
    if (kk < 1) {
        set_err("mn_er_candidates: kk must be >= 1 (got %d)", kk);
        return -1;
    }
    if ((long long)n * kk >= (1ll << 31)) {
        set_err("mn_er_candidates: n * kk = %lld entries, 2^31 or more", (long long)n * kk);
        return -1;
    }
    if (dist_threshold != dist_threshold) {
        set_err("mn_er_candidates: dist_threshold is NaN");
        return -1;
    }
    if (n == 0)
        return 0;
    if (er_check_device("mn_er_candidates", device))
        return -1;
    const size_t ne = (size_t)n * kk;
    DevArena A;
    long long *d_ent = er_upload(A, nullptr, (const long long *)ent_ids, (size_t)n);
    long long *d_nids = er_upload(A, nullptr, (const long long *)nbr_ids, ne);
    float *d_nd = er_upload(A, nullptr, nbr_dists, ne);
    int *d_counts = er_upload(A, nullptr, counts, (size_t)n);
    int *d_r1 = A.alloc<int>(ne), *d_r2 = A.alloc<int>(ne);
    double *d_dist = A.alloc<double>(ne);
    if (!d_ent || !d_nids || !d_nd || !d_counts || !d_r1 || !d_r2 || !d_dist) {
        set_err("mn_er_candidates: out of device memory");
        return -1;
    }
    const long long m = er_candidates_dev(A, nullptr, n, kk, d_ent, nullptr, d_nids, d_nd, d_counts, dist_threshold, d_r1, d_r2, d_dist);
    if (m > 0) {
        HIPCHK(hipMemcpy(r1, d_r1, (size_t)m * sizeof(int), hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(r2, d_r2, (size_t)m * sizeof(int), hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(dist, d_dist, (size_t)m * sizeof(double), hipMemcpyDeviceToHost));
    }
    return m;
} MN_GUARD_END(set_err, MN_NOTHING, -1)

static int er_check_score_args(const char *fn, int guard, double jw_weight, double match_threshold) {
    if (guard != MN_ER_GUARD_NONE && guard != MN_ER_GUARD_SAME_SOURCE && guard != MN_ER_GUARD_DIFF_TYPE) {
        set_err("%s: unknown type guard %d", fn, guard);
        return -1;
    }
    if (jw_weight != jw_weight) {
        set_err("%s: jw_weight is NaN", fn);
        return -1;
    }
    if (match_threshold != match_threshold) {
        set_err("%s: match_threshold is NaN", fn);
        return -1;
    }
    return 0;
}

extern "C" int64_t mn_er_score(int64_t n_cand, const int *r1, const int *r2, const double *dist, int n, const unsigned char *bytes,
                               const int64_t *off, const int *source_id, int guard, double jw_weight, double match_threshold,
                               int device, mn_er_edge *edges) try {
    if (n_cand < 0 || n < 0 || n_cand >= (1ll << 31) || (n_cand && (!r1 || !r2 || !dist || !edges))) {
        set_err("mn_er_score: bad arguments");
        return -1;
    }
    if (er_check_names("mn_er_score", bytes, off, n) || er_check_score_args("mn_er_score", guard, jw_weight, match_threshold))
        return -1;
    for (int64_t c = 0; c < n_cand; c++)
        if (r1[c] < 0 || r1[c] >= n || r2[c] < 0 || r2[c] >= n) {
            set_err("mn_er_score: candidate %lld names an entity outside [0, %d)", (long long)c, n);
            return -1;
        }
    if (n_cand == 0)
        return 0;
    if (er_check_device("mn_er_score", device))
        return -1;
    DevArena A;
    int *d_r1 = er_upload(A, nullptr, r1, (size_t)n_cand), *d_r2 = er_upload(A, nullptr, r2, (size_t)n_cand);
    double *d_dist = er_upload(A, nullptr, dist, (size_t)n_cand);
    unsigned char *d_bytes = er_upload(A, nullptr, bytes, (size_t)off[n]);
    long long *d_off = er_upload(A, nullptr, (const long long *)off, (size_t)n + 1);
    int *d_src = source_id ? er_upload(A, nullptr, source_id, (size_t)n) : nullptr;
    mn_er_edge *d_edges = A.alloc<mn_er_edge>((size_t)n_cand);
    if (!d_r1 || !d_r2 || !d_dist || !d_bytes || !d_off || (source_id && !d_src) || !d_edges) {
        set_err("mn_er_score: out of device memory");
        return -1;
    }
    const long long m = er_score_dev(A, nullptr, n_cand, d_r1, d_r2, d_dist, d_bytes, d_off, d_src, guard, jw_weight, match_threshold,
                                     d_edges, nullptr);
    if (m > 0)
        HIPCHK(hipMemcpy(edges, d_edges, (size_t)m * sizeof(mn_er_edge), hipMemcpyDeviceToHost));
    return m;
} MN_GUARD_END(set_err, MN_NOTHING, -1)

// the largest float not above t: for every float d, d <= that float exactly when !((double)d > t)
static float er_float_cut(double t) {
    float f = (float)t;
    if ((double)f > t)
        f = nextafterf(f, -INFINITY);
    return f;
}

struct ErEvents {
    hipEvent_t e[4] = {nullptr, nullptr, nullptr, nullptr};
    ~ErEvents() {
        for (hipEvent_t v : e)
            if (v)
                (void)hipEventDestroy(v);
    }
};

extern "C" int64_t mn_hnsw_er_edges(mn_index *x, int n, const int64_t *ent_ids, const unsigned char *bytes, const int64_t *off,
                                    const int *source_id, int k, double dist_threshold, double jw_weight, double match_threshold,
                                    int guard, int blocking, mn_er_edge *edges, mn_er_stats *stats) try {
    if (stats)
        memset(stats, 0, sizeof(*stats));
    if (n < 0 || (n && (!ent_ids || !edges))) {
        set_err("mn_hnsw_er_edges: bad arguments");
        return -1;
    }
    if (k < 1 || k > 127) {
        set_err("mn_hnsw_er_edges: k must be 1..127 (got %d): the searches answer at most 128 and the reference asks for k + 1", k);
        return -1;
    }
    if (blocking != MN_ER_GRAPH && blocking != MN_ER_EXACT) {
        set_err("mn_hnsw_er_edges: unknown blocking %d", blocking);
        return -1;
    }
    if (dist_threshold != dist_threshold) {
        set_err("mn_hnsw_er_edges: dist_threshold is NaN");
        return -1;
    }
    if (er_check_names("mn_hnsw_er_edges", bytes, off, n) || er_check_score_args("mn_hnsw_er_edges", guard, jw_weight, match_threshold))
        return -1;
    const int kk = blocking == MN_ER_GRAPH ? k + 1 : k; // :221-222
    if ((long long)n * kk >= (1ll << 31)) {
        set_err("mn_hnsw_er_edges: n * (k + 1) = %lld entries, 2^31 or more", (long long)n * kk);
        return -1;
    }
    if (!x) { // (after the checks that need no index)
        set_err("mn_hnsw_er_edges: no index");
        return -1;
    }
    if (n == 0)
        return 0;
    if (use_device(x))
        return -1;
    if (push_links(x) || sync_meta(x))
        return -1;
    hipStream_t st = x->stream;
    // row_of[i]: the row of the blocking's answer that is entity i's list — GRAPH: its place among the queries, EXACT: its slot;
    // -1: an absent or deleted row has no vector, the reference's SELECT finds none (:240-243)
    std::vector<int> row_of((size_t)n), qslot;
    for (int i = 0; i < n; i++) {
        int s = ht_find(x, ent_ids[i]);
        if (s >= 0 && x->deleted[(size_t)s])
            s = -1;
        if (blocking == MN_ER_GRAPH && s >= 0) {
            qslot.push_back(s);
            s = (int)qslot.size() - 1;
        }
        row_of[(size_t)i] = s;
    }
    const int nq = (int)qslot.size();
    ErEvents ev;
    for (hipEvent_t &e : ev.e)
        HIPCHK(hipEventCreate(&e));
    DevArena A;
    const size_t rows = (size_t)std::max(1, blocking == MN_ER_GRAPH ? nq : x->n_slots);
    long long *d_ent = er_upload(A, st, (const long long *)ent_ids, (size_t)n);
    int *d_row_of = er_upload(A, st, row_of.data(), (size_t)n);
    unsigned char *d_bytes = er_upload(A, st, bytes, (size_t)off[n]);
    long long *d_off = er_upload(A, st, (const long long *)off, (size_t)n + 1);
    int *d_src = source_id ? er_upload(A, st, source_id, (size_t)n) : nullptr;
    long long *d_nids = A.alloc<long long>(rows * kk);
    float *d_nd = A.alloc<float>(rows * kk);
    int *d_counts = A.alloc<int>(rows);
    int *d_r1 = A.alloc<int>((size_t)n * kk), *d_r2 = A.alloc<int>((size_t)n * kk);
    double *d_dist = A.alloc<double>((size_t)n * kk);
    unsigned long long *d_path = A.alloc<unsigned long long>(2);
    if (!d_ent || !d_row_of || !d_bytes || !d_off || (source_id && !d_src) || !d_nids || !d_nd || !d_counts || !d_r1 || !d_r2 || !d_dist ||
        !d_path) {
        set_err("mn_hnsw_er_edges: out of device memory");
        return -1;
    }
    HIPCHK(hipMemsetAsync(d_path, 0, 2 * sizeof(unsigned long long), st));
    HIPCHK(hipMemsetAsync(d_counts, 0, rows * sizeof(int), st));
    HIPCHK(hipEventRecord(ev.e[0], st));
    if (blocking == MN_ER_GRAPH && nq > 0) {
        // hnsw_vtab.c:591: a MATCH without ef_search searches with ef = 2 * k, k being the statement's k + 1
        float *d_q = A.alloc<float>((size_t)nq * x->dim);
        int *d_qslot = er_upload(A, st, qslot.data(), (size_t)nq);
        if (!d_q || !d_qslot) {
            set_err("mn_hnsw_er_edges: out of device memory");
            return -1;
        }
        hipLaunchKernelGGL(k_er_gather, ER_GRID((long long)nq * x->dim, 256), dim3(256), 0, st, x->d_vectors.p, x->ld, x->dim, d_qslot, nq,
                           d_q);
        if (mn_hnsw_search_batch_dev(x, d_q, nq, kk, 2 * kk, (int64_t *)d_nids, d_nd, d_counts))
            return -1;
        long long n_overflow = 0; // a truncated list must not become candidates silently: mn_hnsw_search_batch fails here too
        if (mn_index_search_overflow(x, &n_overflow))
            return -1;
        if (n_overflow) {
            set_err("mn_hnsw_er_edges: %lld queries exceeded heap workspace", n_overflow);
            return -1;
        }
    } else if (blocking == MN_ER_EXACT && x->n_slots > 0) {
        if (mn_hnsw_knn_graph_dev(x, kk, er_float_cut(dist_threshold), (int64_t *)d_nids, d_nd, d_counts))
            return -1;
    }
    HIPCHK(hipEventRecord(ev.e[1], st));
    const long long n_cand = er_candidates_dev(A, st, n, kk, d_ent, d_row_of, d_nids, d_nd, d_counts, dist_threshold, d_r1, d_r2, d_dist);
    if (n_cand < 0)
        return -1;
    HIPCHK(hipEventRecord(ev.e[2], st));
    mn_er_edge *d_edges = A.alloc<mn_er_edge>((size_t)std::max<long long>(1, n_cand));
    if (!d_edges) {
        set_err("mn_hnsw_er_edges: out of device memory");
        return -1;
    }
    const long long n_edges = er_score_dev(A, st, n_cand, d_r1, d_r2, d_dist, d_bytes, d_off, d_src, guard, jw_weight, match_threshold,
                                           d_edges, d_path);
    if (n_edges < 0)
        return -1;
    HIPCHK(hipEventRecord(ev.e[3], st));
    unsigned long long path[2] = {0, 0};
    HIPCHK(hipMemcpyAsync(path, d_path, sizeof(path), hipMemcpyDeviceToHost, st));
    if (n_edges > 0)
        HIPCHK(hipMemcpyAsync(edges, d_edges, (size_t)n_edges * sizeof(mn_er_edge), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (stats) {
        float ms = 0;
        stats->n_candidates = n_cand;
        stats->n_edges = n_edges;
        stats->n_jw_short = (int64_t)path[0];
        stats->n_jw_long = (int64_t)path[1];
        if (hipEventElapsedTime(&ms, ev.e[0], ev.e[1]) == hipSuccess)
            stats->blocking_ms = ms;
        if (hipEventElapsedTime(&ms, ev.e[1], ev.e[2]) == hipSuccess)
            stats->candidates_ms = ms;
        if (hipEventElapsedTime(&ms, ev.e[2], ev.e[3]) == hipSuccess)
            stats->score_ms = ms;
    }
    return n_edges;
} MN_GUARD_END(set_err, MN_NOTHING, -1)
