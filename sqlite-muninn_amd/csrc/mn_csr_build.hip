// mn_csr_build.hip — the mn_graph handle built on the device from an edge list, and read back.
//
// mn_graph_from_edges replaces the reference's two host steps: the ingest loop's adj_add per row (src/graph_load.c:227-246:
// out[src] gets dst, in[dst] gets src, in row order) and csr_build over the lists it made (src/graph_csr.c:20-83).  A CSR
// list in row order is the list's row numbers in ascending order, so the build is
//   1. k_count     one lane per row: range check, 32-bit atomicAdd into the degree counters of both directions
//   2. scan        rocprim::exclusive_scan → offsets
//   3. k_fill      one lane per row takes a slot of its list (atomicSub on the same counter) and stores its ROW NUMBER: the
//                  only step whose result depends on arrival order
//   4. sort        every list's row numbers ascending.  They are unique, so what step 3 left behind no longer shows.  Lists
//                  are binned by degree on the host (it needs the offsets anyway): up to MN_CSR_SORT_WAVE (64) entries a
//                  bitonic network in registers, 8 / 16 / 32 / 64 lanes per list; up to MN_CSR_SORT_LDS (8192) a workgroup's
//                  bitonic sort in LDS; longer ones one rocprim::segmented_radix_sort_keys over just those lists
//   5. k_gather    targets and weights through the sorted row numbers (weights move as 64-bit words: NaN payloads stay)
// MN_CSR_BUILD=radix replaces 3 and 4 by one stable rocprim::radix_sort_pairs of (node, row number): the second,
// independent implementation the tests hold the first against, and its baseline.  Both give the same bytes.  On the 1M-node /
// 20M-row benchmark graph (bench_adjacency.py, README) the radix route is the faster one, so it is the default and
// MN_CSR_BUILD=sort selects steps 3 and 4.
// mn_graph_export_csr is csr_build's result as the host sees it; mn_graph_retain lets a second owner keep the handle.
#include "mn_graph_int.hpp"
#include "mn_guard.hpp"

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>
#include <rocprim/device/device_segmented_radix_sort.hpp>
#include <rocprim/iterator/counting_iterator.hpp>

#include <climits>
#include <cstring>

namespace {

constexpr int kBlock = 256;
constexpr int kLdsMax = 8192; // ints a workgroup sorts in LDS (32 KiB)
constexpr int kWaveMax = 64;

inline unsigned grid_for(long long items) {
    const long long b = (items + kBlock - 1) / kBlock;
    return (unsigned)std::max<long long>(1, std::min<long long>(b, 256 * 16)); // grid-stride beyond 16 blocks per CU
}

// 1. degrees of both directions in one pass.  A row with an index outside 0 .. n - 1 adds nothing anywhere and leaves its
// number in *bad (the smallest such row wins, so the message does not depend on arrival order).
__global__ __launch_bounds__(kBlock) void k_count(int n, int E, const int *__restrict__ src, const int *__restrict__ dst, int lists,
                                                  int *cnt_out, int *cnt_in, int *bad) {
    const long long stride = (long long)gridDim.x * kBlock;
    for (long long r = (long long)blockIdx.x * kBlock + threadIdx.x; r < E; r += stride) {
        const int s = src[r], d = dst[r];
        if ((unsigned)s >= (unsigned)n || (unsigned)d >= (unsigned)n) {
            atomicMin(bad, (int)r);
            continue;
        }
        if (lists & 1)
            atomicAdd(&cnt_out[s], 1);
        if (lists & 2)
            atomicAdd(&cnt_in[d], 1);
    }
}

// 3. every row takes one slot of its list: the counter of k_count goes back down to zero, so slot = off + 0 .. degree - 1,
// each exactly once.  Runs only after k_count found every index in range.
__global__ __launch_bounds__(kBlock) void k_fill(int E, const int *__restrict__ src, const int *__restrict__ dst, int lists,
                                                 int *cnt_out, int *cnt_in, const int *__restrict__ off_out,
                                                 const int *__restrict__ off_in, int *rows_out, int *rows_in) {
    const long long stride = (long long)gridDim.x * kBlock;
    for (long long r = (long long)blockIdx.x * kBlock + threadIdx.x; r < E; r += stride) {
        if (lists & 1) {
            const int s = src[r];
            rows_out[off_out[s] + atomicSub(&cnt_out[s], 1) - 1] = (int)r;
        }
        if (lists & 2) {
            const int d = dst[r];
            rows_in[off_in[d] + atomicSub(&cnt_in[d], 1) - 1] = (int)r;
        }
    }
}

// 4a. lists of at most W entries, W lanes each: a bitonic network through __shfl_xor.  Lanes beyond the list hold INT_MAX,
// which is no row number (n_rows < INT_MAX) and sorts behind every one.  Every lane of the wave takes part in every shuffle.
template <int W>
__global__ __launch_bounds__(kBlock) void k_sort_reg(const int *__restrict__ nodes, int count, const int *__restrict__ off, int *rows) {
    const long long gid = ((long long)blockIdx.x * kBlock + threadIdx.x) / W;
    const int l = threadIdx.x % W;
    int base = 0, d = 0;
    if (gid < count) {
        const int v = nodes[gid];
        base = off[v];
        d = off[v + 1] - base;
        if (d > W)
            d = 0; // not this kernel's list (the host bins by degree; never taken)
    }
    int x = l < d ? rows[base + l] : INT_MAX;
#pragma unroll
    for (int k = 2; k <= W; k <<= 1) {
#pragma unroll
        for (int j = k >> 1; j > 0; j >>= 1) {
            const int y = __shfl_xor(x, j, W);
            const bool up = (l & k) == 0, lo = (l & j) == 0;
            x = (lo == up) ? min(x, y) : max(x, y);
        }
    }
    if (l < d)
        rows[base + l] = x;
}

// 4b. one workgroup per list of at most kLdsMax entries: bitonic sort in LDS over the next power of two, padded with INT_MAX.
__global__ __launch_bounds__(kBlock) void k_sort_lds(const int *__restrict__ nodes, const int *__restrict__ off, int *rows) {
    __shared__ int s[kLdsMax];
    const int v = nodes[blockIdx.x];
    const int base = off[v];
    int d = off[v + 1] - base;
    if (d > kLdsMax)
        d = 0; // never taken: see k_sort_reg
    int P = 2;
    while (P < d)
        P <<= 1;
    for (int i = threadIdx.x; i < P; i += kBlock)
        s[i] = i < d ? rows[base + i] : INT_MAX;
    __syncthreads();
    for (int k = 2; k <= P; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = threadIdx.x; i < P; i += kBlock) {
                const int p = i ^ j;
                if (p > i) {
                    const int a = s[i], b = s[p];
                    if ((a > b) == ((i & k) == 0)) {
                        s[i] = b;
                        s[p] = a;
                    }
                }
            }
            __syncthreads();
        }
    }
    for (int i = threadIdx.x; i < d; i += kBlock)
        rows[base + i] = s[i];
}

// 4c. the long lists come back from the segmented sort's output buffer, one workgroup per list
__global__ __launch_bounds__(kBlock) void k_copy_segments(const int *__restrict__ seg_begin, const int *__restrict__ seg_end,
                                                          const int *__restrict__ from, int *to) {
    const int b = seg_begin[blockIdx.x], e = seg_end[blockIdx.x];
    for (int i = b + threadIdx.x; i < e; i += kBlock)
        to[i] = from[i];
}

// 5. slot i lists what row rows[i] names
__global__ __launch_bounds__(kBlock) void k_gather(int E, const int *__restrict__ rows, const int *__restrict__ val,
                                                   const unsigned long long *__restrict__ w, int *tgt, unsigned long long *w_dst) {
    const long long stride = (long long)gridDim.x * kBlock;
    for (long long i = (long long)blockIdx.x * kBlock + threadIdx.x; i < E; i += stride) {
        const int r = rows[i];
        tgt[i] = val[r];
        if (w)
            w_dst[i] = w[r];
    }
}

int env_int(const char *name, int dflt, int lo, int hi) {
    const char *e = getenv(name);
    if (!e || !*e)
        return dflt;
    const long v = strtol(e, nullptr, 10);
    return (int)std::max<long>(lo, std::min<long>(hi, v));
}

struct Dir {            // one direction under construction
    const int *key;     // the node a row is listed under (device)
    const int *val;     // what the row lists there (device)
    int *cnt;           // n + 1 counters
    int *off;           // the handle's n + 1 offsets
    int *rows;          // E row numbers
    int *tgt;           // the handle's targets (scratch for sorted keys until k_gather)
    double *w;          // the handle's weights or null
    std::vector<int> *h_off;
};

int scan_offsets(DevArena &A, const Dir &d, int n, hipStream_t st) {
    size_t need = 0;
    GCHK(rocprim::exclusive_scan(nullptr, need, d.cnt, d.off, 0, (size_t)n + 1, rocprim::plus<int>(), st));
    void *tmp = A.alloc<char>(need);
    if (!tmp) {
        gset_err("mn_graph_from_edges: out of device memory (scan scratch)");
        return -1;
    }
    GCHK(rocprim::exclusive_scan(tmp, need, d.cnt, d.off, 0, (size_t)n + 1, rocprim::plus<int>(), st));
    return 0;
}

// 4. of the hand-written route, for one direction whose slots k_fill has filled
int sort_lists(DevArena &A, std::vector<std::vector<int>> &keep, const Dir &d, int n, int E, int t_wave, int t_lds, hipStream_t st) {
    const std::vector<int> &off = *d.h_off;
    // bins: 0..3 = 8 / 16 / 32 / 64 lanes in registers, 4 = LDS, 5 = segmented sort; lists of 0 or 1 entries are sorted
    auto bin_of = [&](int deg) {
        if (deg < 2)
            return -1;
        if (deg <= t_wave)
            return deg <= 8 ? 0 : deg <= 16 ? 1 : deg <= 32 ? 2 : 3;
        return deg <= t_lds ? 4 : 5;
    };
    size_t cnt[6] = {0, 0, 0, 0, 0, 0};
    for (int v = 0; v < n; v++) {
        const int b = bin_of(off[(size_t)v + 1] - off[(size_t)v]);
        if (b >= 0)
            cnt[b]++;
    }
    size_t start[7] = {0};
    for (int b = 0; b < 6; b++)
        start[b + 1] = start[b] + cnt[b];
    const size_t total = start[6];
    if (!total)
        return 0;
    keep.emplace_back(total); // what the asynchronous copies below read stays until the caller has waited for the stream
    keep.emplace_back();
    std::vector<int> &nodes = keep[keep.size() - 2], &seg = keep.back();
    size_t pos[6];
    memcpy(pos, start, sizeof(pos));
    for (int v = 0; v < n; v++) {
        const int b = bin_of(off[(size_t)v + 1] - off[(size_t)v]);
        if (b >= 0)
            nodes[pos[b]++] = v;
    }
    int *d_nodes = A.alloc<int>(total);
    if (!d_nodes) {
        gset_err("mn_graph_from_edges: out of device memory (bins)");
        return -1;
    }
    GCHK(hipMemcpyAsync(d_nodes, nodes.data(), total * sizeof(int), hipMemcpyHostToDevice, st));
    auto reg_grid = [](size_t lists, int W) { return (unsigned)((lists * (size_t)W + kBlock - 1) / kBlock); };
    if (cnt[0])
        hipLaunchKernelGGL(k_sort_reg<8>, dim3(reg_grid(cnt[0], 8)), dim3(kBlock), 0, st, d_nodes + start[0], (int)cnt[0], d.off, d.rows);
    if (cnt[1])
        hipLaunchKernelGGL(k_sort_reg<16>, dim3(reg_grid(cnt[1], 16)), dim3(kBlock), 0, st, d_nodes + start[1], (int)cnt[1], d.off, d.rows);
    if (cnt[2])
        hipLaunchKernelGGL(k_sort_reg<32>, dim3(reg_grid(cnt[2], 32)), dim3(kBlock), 0, st, d_nodes + start[2], (int)cnt[2], d.off, d.rows);
    if (cnt[3])
        hipLaunchKernelGGL(k_sort_reg<64>, dim3(reg_grid(cnt[3], 64)), dim3(kBlock), 0, st, d_nodes + start[3], (int)cnt[3], d.off, d.rows);
    if (cnt[4])
        hipLaunchKernelGGL(k_sort_lds, dim3((unsigned)cnt[4]), dim3(kBlock), 0, st, d_nodes + start[4], d.off, d.rows);
    GCHK(hipGetLastError());
    if (cnt[5]) {
        const size_t nl = cnt[5];
        seg.resize(2 * nl);
        for (size_t i = 0; i < nl; i++) {
            const int v = nodes[start[5] + i];
            seg[i] = off[(size_t)v];
            seg[nl + i] = off[(size_t)v + 1];
        }
        int *d_seg = A.alloc<int>(2 * nl);
        if (!d_seg) {
            gset_err("mn_graph_from_edges: out of device memory (segments)");
            return -1;
        }
        GCHK(hipMemcpyAsync(d_seg, seg.data(), 2 * nl * sizeof(int), hipMemcpyHostToDevice, st));
        unsigned bits = 1;
        while (bits < 31 && (1LL << bits) < E)
            bits++;
        size_t need = 0;
        GCHK(rocprim::segmented_radix_sort_keys(nullptr, need, d.rows, d.tgt, (unsigned)E, (unsigned)nl, d_seg, d_seg + nl, 0, bits, st));
        void *tmp = A.alloc<char>(need);
        if (!tmp) {
            gset_err("mn_graph_from_edges: out of device memory (segmented sort scratch)");
            return -1;
        }
        GCHK(rocprim::segmented_radix_sort_keys(tmp, need, d.rows, d.tgt, (unsigned)E, (unsigned)nl, d_seg, d_seg + nl, 0, bits, st));
        hipLaunchKernelGGL(k_copy_segments, dim3((unsigned)nl), dim3(kBlock), 0, st, d_seg, d_seg + nl, d.tgt, d.rows);
        GCHK(hipGetLastError());
    }
    return 0;
}

// 3 + 4 of MN_CSR_BUILD=radix: rows ordered by (node, row number) in one stable sort; the sorted keys land in d.tgt, which
// k_gather overwrites afterwards
int radix_rows(DevArena &A, const Dir &d, int n, int E, hipStream_t st) {
    unsigned bits = 1;
    while (bits < 31 && (1LL << bits) < n)
        bits++;
    rocprim::counting_iterator<int> iota(0);
    size_t need = 0;
    GCHK(rocprim::radix_sort_pairs(nullptr, need, d.key, d.tgt, iota, d.rows, (size_t)E, 0, bits, st));
    void *tmp = A.alloc<char>(need);
    if (!tmp) {
        gset_err("mn_graph_from_edges: out of device memory (radix sort scratch)");
        return -1;
    }
    GCHK(rocprim::radix_sort_pairs(tmp, need, d.key, d.tgt, iota, d.rows, (size_t)E, 0, bits, st));
    return 0;
}

template <typename T> int dev_alloc(T **p, size_t n) {
    *p = nullptr;
    GCHK(hipMalloc(p, (n ? n : 1) * sizeof(T)));
    return 0;
}

int build_into(mn_graph *g, int n, int E, const int *src, const int *dst, const double *w, int lists) {
    GCHK(hipSetDevice(g->device));
    GCHK(hipStreamCreateWithFlags(&g->stream, hipStreamNonBlocking));
    GCHK(hipEventCreate(&g->ev0));
    GCHK(hipEventCreate(&g->ev1));
    hipStream_t st = g->stream;
    const bool radix = [] {
        const char *e = getenv("MN_CSR_BUILD");
        return !(e && strcmp(e, "sort") == 0); // radix unless asked otherwise: the faster one where both were measured
    }();
    const int t_wave = env_int("MN_CSR_SORT_WAVE", kWaveMax, 0, kWaveMax);
    const int t_lds = env_int("MN_CSR_SORT_LDS", kLdsMax, 0, kLdsMax);

    std::vector<std::vector<int>> keep; // host staging of sort_lists: declared first, so it outlives the arena's hipFree
    keep.reserve(4);
    DevArena A;
    int *d_src = A.alloc<int>((size_t)E), *d_dst = A.alloc<int>((size_t)E), *d_bad = A.alloc<int>(1);
    int *cnt_out = A.alloc<int>((size_t)n + 1), *cnt_in = A.alloc<int>((size_t)n + 1);
    double *d_w = w ? A.alloc<double>((size_t)E) : nullptr;
    if (!d_src || !d_dst || !d_bad || !cnt_out || !cnt_in || (w && !d_w)) {
        gset_err("mn_graph_from_edges: out of device memory (%d rows, %d nodes)", E, n);
        return -1;
    }
    if (dev_alloc(&g->off_out, (size_t)n + 1) || dev_alloc(&g->off_in, (size_t)n + 1))
        return -1;
    const int none = INT_MAX;
    if (E) {
        GCHK(hipMemcpyAsync(d_src, src, (size_t)E * sizeof(int), hipMemcpyHostToDevice, st));
        GCHK(hipMemcpyAsync(d_dst, dst, (size_t)E * sizeof(int), hipMemcpyHostToDevice, st));
        if (w)
            GCHK(hipMemcpyAsync(d_w, w, (size_t)E * sizeof(double), hipMemcpyHostToDevice, st));
    }
    GCHK(hipMemcpyAsync(d_bad, &none, sizeof(int), hipMemcpyHostToDevice, st));
    GCHK(hipMemsetAsync(cnt_out, 0, ((size_t)n + 1) * sizeof(int), st));
    GCHK(hipMemsetAsync(cnt_in, 0, ((size_t)n + 1) * sizeof(int), st));
    GCHK(hipEventRecord(g->ev0, st));
    if (E) {
        hipLaunchKernelGGL(k_count, dim3(grid_for(E)), dim3(kBlock), 0, st, n, E, d_src, d_dst, lists, cnt_out, cnt_in, d_bad);
        GCHK(hipGetLastError());
        int bad = INT_MAX;
        GCHK(hipMemcpyAsync(&bad, d_bad, sizeof(int), hipMemcpyDeviceToHost, st));
        GCHK(hipStreamSynchronize(st));
        if (bad != INT_MAX) {
            gset_err("mn_graph_from_edges: row %d names node %d -> %d, outside 0 .. %d", bad, src[bad], dst[bad], n - 1);
            return -1;
        }
    }

    g->h_off_out.assign((size_t)n + 1, 0);
    g->h_off_in.assign((size_t)n + 1, 0);
    g->e_out = (lists & 1) ? E : 0;
    g->e_in = (lists & 2) ? E : 0;
    if (dev_alloc(&g->tgt_out, (size_t)g->e_out) || dev_alloc(&g->tgt_in, (size_t)g->e_in))
        return -1;
    if (w && (lists & 1) && dev_alloc(&g->w_out, (size_t)g->e_out))
        return -1;
    if (w && (lists & 2) && dev_alloc(&g->w_in, (size_t)g->e_in))
        return -1;
    Dir dirs[2] = {{d_src, d_dst, cnt_out, g->off_out, nullptr, g->tgt_out, g->w_out, &g->h_off_out},
                   {d_dst, d_src, cnt_in, g->off_in, nullptr, g->tgt_in, g->w_in, &g->h_off_in}};
    for (int k = 0; k < 2; k++) {
        Dir &d = dirs[k];
        if (!(lists & (1 << k)) || !E) { // a list the graph does not hold, or holds empty: every offset 0
            GCHK(hipMemsetAsync(d.off, 0, ((size_t)n + 1) * sizeof(int), st));
            continue;
        }
        if (!(d.rows = A.alloc<int>((size_t)E))) {
            gset_err("mn_graph_from_edges: out of device memory (row numbers)");
            return -1;
        }
        if (scan_offsets(A, d, n, st))
            return -1;
        GCHK(hipMemcpyAsync(d.h_off->data(), d.off, ((size_t)n + 1) * sizeof(int), hipMemcpyDeviceToHost, st));
    }
    if (E) {
        if (!radix) {
            hipLaunchKernelGGL(k_fill, dim3(grid_for(E)), dim3(kBlock), 0, st, E, d_src, d_dst, lists, cnt_out, cnt_in, g->off_out, g->off_in,
                               dirs[0].rows, dirs[1].rows);
            GCHK(hipGetLastError());
        }
        GCHK(hipStreamSynchronize(st)); // the offsets are on the host from here
        for (int k = 0; k < 2; k++) {
            const Dir &d = dirs[k];
            if (!(lists & (1 << k)))
                continue;
            if (d.h_off->back() != E) {
                gset_err("mn_graph_from_edges: offsets end at %d, not at the %d rows counted", d.h_off->back(), E);
                return -1;
            }
            if (radix ? radix_rows(A, d, n, E, st) : sort_lists(A, keep, d, n, E, t_wave, t_lds, st))
                return -1;
            hipLaunchKernelGGL(k_gather, dim3(grid_for(E)), dim3(kBlock), 0, st, E, d.rows, d.val,
                               reinterpret_cast<const unsigned long long *>(d_w), d.tgt, reinterpret_cast<unsigned long long *>(d.w));
            GCHK(hipGetLastError());
        }
    }
    GCHK(hipEventRecord(g->ev1, st));
    GCHK(hipStreamSynchronize(st));
    graph_note_ms(g);
    g->weighted = w != nullptr;
    for (int v = 0; v < n; v++) {
        const int dO = g->h_off_out[(size_t)v + 1] - g->h_off_out[(size_t)v], dI = g->h_off_in[(size_t)v + 1] - g->h_off_in[(size_t)v];
        g->max_deg_out = std::max(g->max_deg_out, dO);
        g->max_deg_both = std::max(g->max_deg_both, dO + dI);
    }
    return 0;
}

} // namespace

extern "C" mn_graph *mn_graph_from_edges(int n_nodes, int64_t n_rows, const int *src, const int *dst, const double *w, int lists,
                                         int device) try {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) {
        gset_err("mn_graph_from_edges: HIP device %d not available (no CPU fallback)", device);
        return nullptr;
    }
    if (n_rows < 0) {
        gset_err("mn_graph_from_edges: negative row count %lld", (long long)n_rows);
        return nullptr;
    }
    if (n_nodes < 0 || lists < 1 || lists > 3 || (n_rows > 0 && (!src || !dst))) {
        gset_err("mn_graph_from_edges: bad arguments");
        return nullptr;
    }
    if (n_rows >= INT_MAX) { // offsets and row numbers are int32, and INT_MAX pads the sorts
        gset_err("mn_graph_from_edges: %lld rows exceed int32 offsets", (long long)n_rows);
        return nullptr;
    }
    if (n_rows > 0 && n_nodes == 0) {
        gset_err("mn_graph_from_edges: row 0 names node %d -> %d, outside an empty graph", src[0], dst[0]);
        return nullptr;
    }
    mn_graph *g = new mn_graph();
    g->device = device;
    g->n = n_nodes;
    if (build_into(g, n_nodes, (int)n_rows, src, dst, w, lists) != 0) {
        mn_graph_destroy(g);
        return nullptr;
    }
    return g;
} MN_GUARD_END(gset_err, MN_NOTHING, nullptr)

// csr_build's CsrArray (src/graph_csr.c:20-70) of one direction on the host: off[n + 1], tgt[edges], w[edges].  w is filled
// only where the graph holds weights for that direction, and the return value says whether it does (1) or not (0).
extern "C" int mn_graph_export_csr(mn_graph *g, int which, int *off, int *tgt, double *w) try {
    if (!g || which < 0 || which > 1 || !off) {
        gset_err("mn_graph_export_csr: bad arguments");
        return -1;
    }
    GCHK(hipSetDevice(g->device));
    const std::vector<int> &h = which ? g->h_off_in : g->h_off_out;
    const long long e = which ? g->e_in : g->e_out;
    const int *d_tgt = which ? g->tgt_in : g->tgt_out;
    const double *d_w = which ? g->w_in : g->w_out;
    memcpy(off, h.data(), ((size_t)g->n + 1) * sizeof(int));
    if (e && tgt)
        GCHK(hipMemcpy(tgt, d_tgt, (size_t)e * sizeof(int), hipMemcpyDeviceToHost));
    if (e && w && d_w)
        GCHK(hipMemcpy(w, d_w, (size_t)e * sizeof(double), hipMemcpyDeviceToHost));
    return d_w ? 1 : 0;
} MN_GUARD_END(gset_err, MN_NOTHING, -1)
