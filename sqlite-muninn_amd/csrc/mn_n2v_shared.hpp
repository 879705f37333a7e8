// mn_n2v_shared.hpp — MN_N2V_BATCHED over several GPUs (config 4, see muninn_hip.h): the data-parallel exchange by destination
// shard, its kernels, its buffers and mn_node2vec_train_shared.  Included by mn_n2v.hip alone (the entry point uses the unit's
// session entry points and its preamble).
//
// Every rank holds a replica of both matrices and produces the samples of its slice of a batch's walks.  A rank's samples are
// wanted by ONE rank each: the one that owns the sample's target row (positions: the centre row).  Instead of all-gathering
// everything to everybody, a rank sorts its slots by destination shard — a stable one-pass radix sort, so every bucket keeps the
// walk order —, packs the buckets and exchanges them all-to-all: 1 / world of the bytes on the links, and each rank sorts and
// applies 1 / world of the samples.  The slices are contiguous and the received buckets stand in source-rank order = the batch's
// walk order, so a row's additions are the ones, in the order, that one GPU makes.
#pragma once
#include "mn_comm.hpp"
#include "mn_guard.hpp"
#include "mn_n2v_batched.hpp"
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

// the training entry points' preamble (mn_n2v.hip): 1 to go on, else the entry point's result
int n2v_enter(const char *who, int n, const mn_n2v_params *prm, mn_n2v_stats *stats, bool others_ok = true);

__global__ void k_n2v_shard_keys(const int *dest, int n, int rows_per, int world, int *keys, int *vals, int *hist) {
    __shared__ int h[65];
    for (int i = threadIdx.x; i <= world; i += blockDim.x)
        h[i] = 0;
    __syncthreads();
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < (size_t)n) {
        const int d = dest[i];
        const int k = d < 0 ? world : d / rows_per; // (unused slot: sorts to the end, is not sent)
        keys[i] = k;
        vals[i] = (int)i;
        atomicAdd(&h[k], 1);
    }
    __syncthreads();
    for (int i = threadIdx.x; i <= world; i += blockDim.x)
        if (h[i])
            atomicAdd(&hist[i], h[i]);
}
__global__ void k_n2v_pack_samples(const int *order, int n, const int *c, const int *t, const float *e, int *out) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)n)
        return;
    const int j = order[i];
    out[3 * i] = c[j];
    out[3 * i + 1] = t[j];
    out[3 * i + 2] = __float_as_int(e[j]);
}
__global__ void k_n2v_unpack_samples(const int *in, int n, int *c, int *t, float *e) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)n)
        return;
    c[i] = in[3 * i];
    t[i] = in[3 * i + 1];
    e[i] = __int_as_float(in[3 * i + 2]);
}
// a position travels as one record: its centre, then its neu1e vector
__global__ void __launch_bounds__(64) k_n2v_pack_positions(const int *order, const int *pc, const float *pn, int dim, float *out) {
    const int j = order[blockIdx.x];
    float *o = out + (size_t)blockIdx.x * (dim + 1);
    if (threadIdx.x == 0)
        o[0] = __int_as_float(pc[j]);
    for (int d = threadIdx.x; d < dim; d += 64)
        o[1 + d] = pn[(size_t)j * dim + d];
}
__global__ void __launch_bounds__(64) k_n2v_unpack_positions(const float *in, int dim, int *pc, float *pn) {
    const float *r = in + (size_t)blockIdx.x * (dim + 1);
    if (threadIdx.x == 0)
        pc[blockIdx.x] = __float_as_int(r[0]);
    for (int d = threadIdx.x; d < dim; d += 64)
        pn[(size_t)blockIdx.x * dim + d] = r[1 + d];
}

// One call's state: who this rank is, the buffers of the exchange, and the failure it has yet to tell its peers of.
struct N2vExchange {
    mn_comm *c = nullptr;
    mn_n2v_session *S = nullptr;
    int world = 1, rank = 0;
    int rows_per = 0;   // destination rows per rank (equal shards: the last one is padded)
    int shard_bits = 1; // key bits of the bucket sort
    DevArena mem;
    int *lc = nullptr, *lt = nullptr, *lpc = nullptr; // this rank's slice of the batch, as n2v_samples leaves it
    float *le = nullptr, *lpn = nullptr;
    int *send_s = nullptr, *recv_s = nullptr; // packed buckets out and in
    float *send_p = nullptr, *recv_p = nullptr;
    int *gc = nullptr, *gt = nullptr, *gpc = nullptr; // what this rank's rows receive, unpacked
    float *ge = nullptr, *gpn = nullptr;
    int *d_hist = nullptr; // [2][65] bucket sizes: samples, positions
    long long *d_cnt = nullptr;
    char *tmp = nullptr; // the bucket sort's scratch: the session's, or the call's own when that one is too small
    size_t tmp_bytes = 0;
    std::vector<int> h_hist;
    std::vector<long long> h_cnt, h_row;
    // A rank whose local step fails may not leave the loop on its own: its peers are in — or about to enter — the batch's
    // all-gathers and would wait for ever.  `status` carries a local failure (this batch's samples, or the previous batch's
    // apply) into the status exchange at the head of the next collective; all ranks stop together (mn_comm_agree).
    int status = 0;
    std::string mine;
    void fail() {
        status = 1;
        mine = mn_node2vec_last_error();
    }
    ~N2vExchange() { (void)hipDeviceSynchronize(); } // (before `mem` frees what the stream may still be using)
};

static int n2v_exchange_init(N2vExchange &x, mn_comm *c, mn_n2v_session *S) {
    x.c = c;
    x.S = S;
    x.world = c ? c->world : 1;
    x.rank = c ? c->rank : 0;
    const int world = x.world, dim = S->a.dim;
    if (world > 64) {
        nset_err("mn_node2vec_train_shared: more than 64 ranks");
        return -1;
    }
    x.rows_per = (S->a.n + world - 1) / world;
    const int per_max = (S->B + world - 1) / world;
    const size_t ls = (size_t)per_max * S->cap, lp = (size_t)per_max * S->a.walk_length;
    DevArena &m = x.mem;
    bool ok = (x.lc = m.alloc<int>(ls)) && (x.lt = m.alloc<int>(ls)) && (x.le = m.alloc<float>(ls)) && (x.lpc = m.alloc<int>(lp)) &&
              (x.lpn = m.alloc<float>(lp * dim));
    if (ok && world > 1) // the exchange by destination shard: packed buckets out, packed buckets in, then the unpacked arrays
        ok = (x.send_s = m.alloc<int>(ls * 3)) && (x.recv_s = m.alloc<int>(ls * world * 3)) &&
             (x.send_p = m.alloc<float>(lp * (dim + 1))) && (x.recv_p = m.alloc<float>(lp * world * (dim + 1))) &&
             (x.gc = m.alloc<int>(ls * world)) && (x.gt = m.alloc<int>(ls * world)) && (x.ge = m.alloc<float>(ls * world)) &&
             (x.gpc = m.alloc<int>(lp * world)) && (x.gpn = m.alloc<float>(lp * world * dim)) &&
             (x.d_hist = m.alloc<int>(2 * 65)) && (x.d_cnt = m.alloc<long long>((size_t)(world + 1) * 2 * world));
    if (!ok) {
        nset_err("mn_node2vec_train_shared: out of device memory for the exchange buffers");
        return -1;
    }
    while ((1 << x.shard_bits) <= world)
        x.shard_bits++;
    x.tmp = S->tmp;
    x.tmp_bytes = S->tmp_bytes;
    if (world > 1) { // the bucket sort's scratch (fewer key bits than the row sorts: its own size query)
        size_t need = 0;
        if (rocprim::radix_sort_pairs(nullptr, need, S->keys, S->keys_s, S->vals, S->vals_s, ls, 0, x.shard_bits, S->st) != hipSuccess) {
            nset_err("rocprim::radix_sort_pairs (size query) failed");
            return -1;
        }
        if (need > S->tmp_bytes) {
            if (!(x.tmp = m.alloc<char>(need))) {
                nset_err("mn_node2vec_train_shared: out of device memory for the sort scratch");
                return -1;
            }
            x.tmp_bytes = need;
        }
    }
    x.h_hist.resize(2 * 65);
    x.h_cnt.resize((size_t)2 * world * world);
    x.h_row.resize((size_t)2 * world);
    return 0;
}

// this rank's slice [lo, hi) of the batch that starts at node b0, `per` walks' worth of slots; a failure is kept in x.status
static void n2v_exchange_samples(N2vExchange &x, int epoch, int w, int b0, int lo, int hi, int per) {
    mn_n2v_session *S = x.S;
    const size_t ls_n = (size_t)per * S->cap, lp_n = (size_t)per * S->a.walk_length;
    // unused slots carry -1 (ranks with a short or empty slice still contribute `per` walks' worth of slots)
    if (hipMemsetAsync(x.lc, 0xFF, ls_n * 4, S->st) != hipSuccess || hipMemsetAsync(x.lt, 0xFF, ls_n * 4, S->st) != hipSuccess ||
        hipMemsetAsync(x.le, 0, ls_n * 4, S->st) != hipSuccess || hipMemsetAsync(x.lpc, 0xFF, lp_n * 4, S->st) != hipSuccess) {
        nset_err("mn_node2vec_train_shared: memset failed");
        x.status = 1;
    } else if (hi > lo && n2v_samples(S, epoch, w, lo, hi, x.lc, x.lt, x.le, x.lpc, x.lpn)) {
        x.status = 1;
    }
    if (const char *fi = getenv("MN_FAULT_INJECT")) { // test hook: "n2v_shared:<rank>:<first node of the batch>"
        int fr = -1, fb = -1;
        if (sscanf(fi, "n2v_shared:%d:%d", &fr, &fb) == 2 && fr == x.rank && fb == b0 && !x.status) {
            nset_err("injected failure (MN_FAULT_INJECT)");
            x.status = 1;
        }
    }
    if (x.status)
        x.fail();
}

// the status exchange every rank enters: 0 when all are well, else the error string is set and all stop with -1
static int n2v_exchange_agree(N2vExchange &x) {
    if (x.world == 1)
        return x.status ? -1 : 0;
    int failed = -1;
    const int ag = mn_comm_agree(x.c, x.status, x.S->st, &failed);
    if (ag == 0)
        return 0;
    if (ag < 0)
        nset_err("mn_node2vec_train_shared: %s", mn_comm_last_error_str());
    else if (failed == x.rank)
        nset_err("mn_node2vec_train_shared: rank %d failed: %s", x.rank, x.mine.c_str());
    else
        nset_err("mn_node2vec_train_shared: rank %d failed; all ranks stop", failed);
    return -1;
}

// Sorts this rank's ls_n sample slots by the shard of their target row and its lp_n position slots by the shard of their centre
// row, packs the buckets into send_s / send_p and leaves the bucket sizes in h_hist ([0..world]: samples, [65..65+world]:
// positions; the last bucket of each is the unused slots).  False when a step failed.
static bool n2v_exchange_buckets(N2vExchange &x, int ls_n, int lp_n) {
    mn_n2v_session *S = x.S;
    const int world = x.world, dim = S->a.dim;
    if (hipMemsetAsync(x.d_hist, 0, 2 * 65 * sizeof(int), S->st) != hipSuccess)
        return false;
    size_t tb = x.tmp_bytes;
    hipLaunchKernelGGL(k_n2v_shard_keys, dim3((ls_n + 255) / 256), dim3(256), 0, S->st, x.lt, ls_n, x.rows_per, world, S->keys, S->vals,
                       x.d_hist);
    if (rocprim::radix_sort_pairs(x.tmp, tb, S->keys, S->keys_s, S->vals, S->vals_s, (size_t)ls_n, 0, x.shard_bits, S->st) != hipSuccess ||
        hipMemcpyAsync(x.h_hist.data(), x.d_hist, 2 * 65 * sizeof(int), hipMemcpyDeviceToHost, S->st) != hipSuccess ||
        hipStreamSynchronize(S->st) != hipSuccess)
        return false;
    const int nv_s = ls_n - x.h_hist[(size_t)world];
    if (nv_s > 0)
        hipLaunchKernelGGL(k_n2v_pack_samples, dim3((nv_s + 255) / 256), dim3(256), 0, S->st, S->vals_s, nv_s, x.lc, x.lt, x.le, x.send_s);
    hipLaunchKernelGGL(k_n2v_shard_keys, dim3((lp_n + 255) / 256), dim3(256), 0, S->st, x.lpc, lp_n, x.rows_per, world, S->keys, S->vals,
                       x.d_hist + 65);
    tb = x.tmp_bytes;
    if (rocprim::radix_sort_pairs(x.tmp, tb, S->keys, S->keys_c, S->vals, S->vals_s, (size_t)lp_n, 0, x.shard_bits, S->st) != hipSuccess ||
        hipMemcpyAsync(x.h_hist.data() + 65, x.d_hist + 65, 65 * sizeof(int), hipMemcpyDeviceToHost, S->st) != hipSuccess ||
        hipStreamSynchronize(S->st) != hipSuccess)
        return false;
    const int nv_p = lp_n - x.h_hist[(size_t)65 + world];
    if (nv_p > 0)
        hipLaunchKernelGGL(k_n2v_pack_positions, dim3(nv_p), dim3(64), 0, S->st, S->vals_s, x.lpc, x.lpn, dim, x.send_p);
    return hipGetLastError() == hipSuccess;
}

// One batch after the ranks have agreed to go on: bucket, count, exchange, unpack, apply, gather the updated shards.  -1 (error
// string set) when a collective failed or a peer could not prepare: all ranks stop.  A failure of this rank's apply is kept in
// x.status for the next agreement.
static int n2v_exchange_batch(N2vExchange &x, int per) {
    mn_n2v_session *S = x.S;
    mn_comm *c = x.c;
    const int world = x.world, rank = x.rank, rows_per = x.rows_per, dim = S->a.dim;
    const int ls_n = per * S->cap, lp_n = per * S->a.walk_length;
    if (world == 1) {
        if (n2v_apply(S, x.lc, x.lt, x.le, ls_n, x.lpc, x.lpn, lp_n, 0, S->a.n))
            x.fail();
        return 0;
    }
    // ── exchange by destination shard: a sample goes to the rank that owns its target row, a position to the one that
    //    owns its centre row; each rank then sorts and applies only what is meant for its rows ──
    const bool xok = n2v_exchange_buckets(x, ls_n, lp_n);
    // the bucket sizes of every rank; a rank whose preparation failed says so in its row (-1) instead of staying
    // away from the collective its peers are about to enter
    for (int p = 0; p < world; p++) {
        x.h_row[(size_t)p] = xok ? x.h_hist[(size_t)p] : -1;
        x.h_row[(size_t)world + p] = xok ? x.h_hist[(size_t)65 + p] : -1;
    }
    long long *d_row = x.d_cnt + (size_t)2 * world * world; // (send and receive areas do not overlap)
    if (hipMemcpyAsync(d_row, x.h_row.data(), (size_t)2 * world * sizeof(long long), hipMemcpyHostToDevice, S->st) != hipSuccess ||
        hipStreamSynchronize(S->st) != hipSuccess ||
        mn_comm_allgather_dev(c, d_row, x.d_cnt, (size_t)2 * world * sizeof(long long), S->st) ||
        hipMemcpyAsync(x.h_cnt.data(), x.d_cnt, (size_t)2 * world * world * sizeof(long long), hipMemcpyDeviceToHost, S->st) != hipSuccess ||
        hipStreamSynchronize(S->st) != hipSuccess) {
        nset_err("mn_node2vec_train_shared: exchanging the bucket sizes failed (%s)", mn_comm_last_error_str());
        return -1;
    }
    for (int sr = 0; sr < world; sr++)
        if (x.h_cnt[(size_t)sr * 2 * world] < 0) {
            nset_err("mn_node2vec_train_shared: rank %d could not prepare its buckets; all ranks stop", sr);
            return -1;
        }
    std::vector<long long> cs((size_t)world * world), cp((size_t)world * world);
    long long ns_recv = 0, np_recv = 0;
    for (int sr = 0; sr < world; sr++)
        for (int p = 0; p < world; p++) {
            cs[(size_t)sr * world + p] = x.h_cnt[(size_t)sr * 2 * world + p];
            cp[(size_t)sr * world + p] = x.h_cnt[(size_t)sr * 2 * world + world + p];
            if (p == rank) {
                ns_recv += cs[(size_t)sr * world + p];
                np_recv += cp[(size_t)sr * world + p];
            }
        }
    if (mn_comm_alltoallv_dev(c, x.send_s, x.recv_s, cs.data(), 12, S->st) ||
        mn_comm_alltoallv_dev(c, x.send_p, x.recv_p, cp.data(), (size_t)(dim + 1) * 4, S->st)) {
        nset_err("mn_node2vec_train_shared: %s", mn_comm_last_error_str());
        return -1;
    }
    if (ns_recv > 0)
        hipLaunchKernelGGL(k_n2v_unpack_samples, dim3((unsigned)((ns_recv + 255) / 256)), dim3(256), 0, S->st, x.recv_s, (int)ns_recv, x.gc,
                           x.gt, x.ge);
    if (np_recv > 0)
        hipLaunchKernelGGL(k_n2v_unpack_positions, dim3((unsigned)np_recv), dim3(64), 0, S->st, x.recv_p, dim, x.gpc, x.gpn);
    // this rank's rows receive exactly the additions, in exactly the order, one GPU gives them; the updated shards of
    // both matrices are all-gathered in place
    if (n2v_apply(S, x.gc, x.gt, x.ge, ns_recv, x.gpc, x.gpn, np_recv, rank * rows_per, (rank + 1) * rows_per))
        x.fail(); // (reported to the peers at the head of the next batch, or after the last one)
    if (mn_comm_allgather_dev(c, S->syn1 + (size_t)rank * rows_per * dim, S->syn1, (size_t)rows_per * dim * 4, S->st) ||
        mn_comm_allgather_dev(c, S->syn0 + (size_t)rank * rows_per * dim, S->syn0, (size_t)rows_per * dim * 4, S->st)) {
        nset_err("mn_node2vec_train_shared: %s", mn_comm_last_error_str());
        return -1;
    }
    return 0;
}

extern "C" int mn_node2vec_train_shared(mn_comm *c, int n, const int *off, const int *adj, const mn_n2v_params *prm, int device,
                                        float *out, mn_n2v_stats *stats) try {
    const int pre = n2v_enter("mn_node2vec_train_shared", n, prm, stats);
    if (pre <= 0)
        return pre;
    N2vSessionPtr S(mn_n2v_begin(n, off, adj, prm, device));
    if (!S)
        return -1;
    N2vExchange x; // (after S: its buffers go first)
    if (n2v_exchange_init(x, c, S.get()) != 0)
        return -1;
    const int B = S->B, world = x.world;
    int rc = 0;
    for (int epoch = 0; epoch < prm->epochs && rc == 0; epoch++)
        for (int w = 0; w < prm->num_walks && rc == 0; w++)
            for (int b0 = 0; b0 < n && rc == 0; b0 += B) {
                const int b1 = std::min(n, b0 + B);
                const int per = (b1 - b0 + world - 1) / world;
                const int lo = std::min(b1, b0 + x.rank * per), hi = std::min(b1, lo + per);
                if (!x.status)
                    n2v_exchange_samples(x, epoch, w, b0, lo, hi, per);
                rc = n2v_exchange_agree(x);
                if (rc == 0)
                    rc = n2v_exchange_batch(x, per);
            }
    if (rc == 0)
        rc = n2v_exchange_agree(x);
    if (rc == 0)
        rc = mn_n2v_finish(S.get(), out, stats);
    return rc < 0 ? -1 : n;
} MN_GUARD_END(nset_err, MN_NOTHING, -1)
