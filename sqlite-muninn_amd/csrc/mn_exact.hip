// mn_exact.hip — exact k-NN over the device-resident index, certified to the bits of the index's own distance (gfx950).
// The product's flat search (mn_hnsw_search_exact_batch); DESIGN.md §3.6 derives the bound and the certificate.
//
//   k_exact_mfma     candidate pass: the query x row block as a GEMM on the f32 matrix cores (v_mfma_f32_32x32x2_f32, the tiling of
//                    k_brute_mfma, mn_brute.hip); the epilogue turns each dot product A into a certified LOWER BOUND lb <= d of the
//                    distance d the index's order computes, and every query keeps the K' = k + slack rows of smallest lb.
//                    K' <= 64: one lane per list entry.
//   k_exact_rescore  one wavefront per query: folds the row chunks' lists, re-scores the K' rows with rows_distance (the index's
//                    inner loop, its bits), sorts by (d, slot) and certifies: with cut = the K'-th lb, every row outside the list
//                    has d >= lb >= cut, so the answer is final when e_k < cut (strict: a row outside with d == e_k and a lower slot
//                    would belong in the answer) or when the list holds every live row.  Other queries are marked.
//   k_exact_valu     the index's inner loop over every live row (k_bruteforce's shape, any k <= 128), with distances and the
//                    (d, slot) tie rule: marked queries gathered into one launch, k > 32, MN_EXACT=valu.
//
// The same three kernels serve the self-join (mn_hnsw_knn_graph) as their SELF = true instantiations: the queries
// are a range of slots of the row store itself (no padded copy), a query never admits its own slot, every list's threshold starts
// at the radius and the answer is cut at d <= r.  SELF is a template parameter: the search flavour compiles without any of it.
#include "mn_dist.hpp"
#include "mn_dispatch.hpp"

#define EX_KMAX 128 // k_exact_valu
typedef float f32x16 __attribute__((ext_vector_type(16)));

#define EX_Q 128
#define EX_R 128
#define EX_KC 32
#define EX_LD 129
// LDS of one k_exact_mfma workgroup (256 threads, 128 queries): two k-major operand stages 2 x 32 x 129 x 4 = 33 024 B, the
// queries' constants, thresholds and counts 128 x (8 + 4 + 4) = 2 048 B, and the lists 128 x K' x 8 B.  K' = 26 (k = 10, slack 16):
// 61 696 B, two workgroups per CU of 160 KB; K' = 64: 100 608 B (asked for per kernel, mn_lds_grant), one workgroup per CU.
static size_t ex_mfma_lds_bytes(int kp) { return (size_t)(2 * EX_KC * EX_LD) * 4 + (size_t)EX_Q * 16 + (size_t)EX_Q * kp * 8; }

struct MnExactArgs {
    const float *q;        // [nq_pad][ld] zero padded (nq_pad multiple of 128)
    const float2 *qc;      // [nq_pad] per-query constants of the bound (k_exact_prep_q)
    const float2 *xc;      // [n_slots] per-row constants (k_exact_prep_rows)
    const unsigned *allow; // slot bitmap or null
    long long nq;
    int k, kp, rows_per_chunk, n_chunks;
    float uc, fl2;         // absolute underflow allowance; L2: 1 - 4γ - 2^-20 rounded down
    float *pd;             // [n_chunks][nq][kp] lower bounds, ascending
    int *pi;               // [n_chunks][nq][kp] slots
    int *pc;               // [n_chunks][nq]
    long long *out_ids;
    float *out_d;
    int *out_cnt;
    unsigned long long *ctr; // [0] marked queries [1] rows re-scored [2] rows whose exact distance lies below their bound
    int *marked;             // [nq] indices of the marked queries, ctr[0] of them
};

// the self-join flavour: query q of the batch is slot s0 + q, and a.q = ix.vectors + s0 * ld
struct MnKnnArgs : MnExactArgs {
    int s0;     // first slot of the batch
    float r;    // the radius: only rows with d <= r are kept (+inf: no cut)
    float thr0; // nextafterf(r, +inf): what every list's threshold starts at (lb < thr0 is lb <= r)
};
template <bool SELF> struct ExArgs { typedef MnExactArgs type; };
template <> struct ExArgs<true> { typedef MnKnnArgs type; };
// k_exact_valu's last argument.  (A wrapper kernel around a shared body would keep the search's argument block as it was, but the
// compiler then allocates the body's registers differently; an empty struct leaves the search's instruction stream bit for bit.)
struct ExNoSelf {};
struct ExSelf {
    int s0;
    float r;
};

DEVI bool ex_row_ok(const MnDevIndex &ix, const unsigned *allow, int row) {
    return !ix.deleted[row] && (!allow || (allow[row >> 5] >> (row & 31) & 1u));
}

// ───────── the constants of the bound, in f64, rounded to the safe side ─────────
// g = γ_{ld+8}; N = Σ x² in f64.  16 lanes per row, float4 each: whole 256-byte segments per load.
//   l2:     x = N (1 - 4g - 8u) rounded down
//   ip:     x = |x| rounded up
//   cosine: x = |x| rounded up, y = 1 / sqrt(nb) rounded up, nb = the stored f32 norm the exact distance divides by (+inf below 2^-40)
__global__ void __launch_bounds__(256) k_exact_prep_rows(MnDevIndex ix, float2 *xc) {
    const int lane16 = threadIdx.x & 15;
    const long long row = ((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 4;
    const bool in = row < ix.n_slots;
    const float *r = ix.vectors + (size_t)(in ? row : 0) * ix.ld;
    double acc = 0.0;
    for (int e = 4 * lane16; e < ix.ld; e += 64) {
        const float4 v = *reinterpret_cast<const float4 *>(r + e);
        acc = fma((double)v.x, (double)v.x, acc);
        acc = fma((double)v.y, (double)v.y, acc);
        acc = fma((double)v.z, (double)v.z, acc);
        acc = fma((double)v.w, (double)v.w, acc);
    }
#pragma unroll
    for (int m = 8; m >= 1; m >>= 1)
        acc += __shfl_xor(acc, m);
    if (!in || lane16 != 0)
        return;
    const double g = mn_gamma(ix.ld + 8), u = 0x1p-24;
    float2 o = make_float2(0.0f, 0.0f);
    if (ix.metric == 0) {
        o.x = __double2float_rd(acc * (1.0 - 4.0 * g - 8.0 * u));
    } else {
        o.x = __double2float_ru(sqrt(acc) * (1.0 + 0x1p-40));
        if (ix.metric == 1) {
            const double s = sqrt((double)ix.norms[row]);
            o.y = s >= 0x1p-40 ? __double2float_ru(1.0 / (s * (1.0 - 0x1p-40))) : __builtin_inff();
        }
    }
    xc[row] = o;
}

// one wavefront per query: the padded copy the GEMM reads, and
//   l2:     x = N (1 - 4g - 8u) rounded down
//   ip:     x = 4g |q| (1 + 2^-20) rounded up
//   cosine: x as ip, y = (1 + 2^-19) / sqrt(na) rounded up, na = |q|² in the index's order (+inf below 2^-40)
// SELF: `queries` is the row store from the batch's first slot on, stride ld, already zero padded; no copy is made (qpad unused).
template <int ORDER, bool SELF = false>
__global__ void __launch_bounds__(64) k_exact_prep_q(MnDevIndex ix, const float *queries, long long nq, float *qpad, float2 *qc) {
    extern __shared__ __align__(16) unsigned char smem[];
    float *q = reinterpret_cast<float *>(smem);
    const int lane = threadIdx.x;
    const long long qi = blockIdx.x;
    const float *src = queries + (size_t)qi * (SELF ? ix.ld : ix.dim);
    double acc = 0.0;
    for (int i = lane; i < ix.ld; i += 64) {
        const float v = (SELF || i < ix.dim) ? src[i] : 0.0f;
        q[i] = v;
        if (!SELF)
            qpad[(size_t)qi * ix.ld + i] = v;
        acc = fma((double)v, (double)v, acc);
    }
    __syncthreads();
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1)
        acc += __shfl_xor(acc, m);
    const double g = mn_gamma(ix.ld + 8), u = 0x1p-24;
    float2 o = make_float2(0.0f, 0.0f);
    if (ix.metric == 0) {
        o.x = __double2float_rd(acc * (1.0 - 4.0 * g - 8.0 * u));
    } else {
        o.x = __double2float_ru(4.0 * g * sqrt(acc) * (1.0 + 0x1p-20));
        if (ix.metric == 1) {
            const double s = sqrt((double)lds_self_norm<ORDER>(q, ix.dim, ix.ld, lane));
            o.y = s >= 0x1p-40 ? __double2float_ru((1.0 + 0x1p-19) / (s * (1.0 - 0x1p-40))) : __builtin_inff();
        }
    }
    if (lane == 0)
        qc[qi] = o;
}

// lb <= d for the pair: A = the approximate dot product, summed in any order.  f32, each rounding allowed for.
template <int METRIC>
DEVI float ex_lower_bound(float A, float2 qc, float2 xc, float uc, float fl2) {
    float lb;
    if (METRIC == 0) {
        const float s = __fsub_rn(__fadd_rn(qc.x, xc.x), __fmul_rn(2.0f, A));
        // s not finite (a_q + a_x or 2A overflows, in either direction; NaN) says nothing about d: a_q + a_x above FLT_MAX leaves
        // d = D - ... anywhere above a_q + a_x - FLT_MAX, finite for near-collinear q and x.  No bound: 0 (a sum of squares is never
        // negative), the row stays a candidate.  (+inf would also never pass `lb < thr` while a list is still filling, thr = +inf,
        // and a list short of K' counts as holding every live row.)
        lb = (s > 0.0f && s < __builtin_inff()) ? fmaxf(__fsub_rn(__fmul_rn(s, fl2), uc), 0.0f) : 0.0f;
        return lb;
    }
    const float t = fmaf(qc.x, xc.x, uc); // >= |dot_ref - A|
    if (METRIC == 2) {
        const float v = __fadd_rn(A, t);
        lb = __fsub_rn(-v, __fmul_rn(fabsf(v), 0x1p-22f));
    } else {
        const float s = fmaxf(__fadd_rn(A, t), 0.0f);
        const float w = __fmul_rn(__fmul_rn(s, qc.y), xc.y); // >= the reference's rounded quotient
        lb = __fsub_rn(1.0f, w);
        lb = __fsub_rn(lb, __fmul_rn(fabsf(lb), 0x1p-22f));
    }
    return lb == lb ? lb : -__builtin_inff();
}

// ───────────────────────── k_exact_mfma ─────────────────────────
// The tile loop of k_brute_mfma: a workgroup (4 wavefronts) owns 128 queries and walks a chunk of the rows 128 at a time; wavefront w
// owns queries 32w..32w+31 against all 128 rows of the tile.  Each (query tile, row chunk) writes one partial list per query.
// SELF: the A operand is the row store itself (a.q = ix.vectors + s0 * ld; a query row at or beyond n_slots, q0 + row >= nq, is
// not read), the pair (query s0 + q, row s0 + q) is never admitted, and the thresholds start at a.thr0.
template <int METRIC, bool SELF = false>
__global__ void __launch_bounds__(256) k_exact_mfma(MnDevIndex ix, typename ExArgs<SELF>::type a) {
    extern __shared__ __align__(16) unsigned char smem[];
    float *As = reinterpret_cast<float *>(smem);           // [EX_KC][EX_LD]
    float *Bs = As + EX_KC * EX_LD;                        // [EX_KC][EX_LD]
    float2 *qc_s = reinterpret_cast<float2 *>(Bs + EX_KC * EX_LD); // [128]
    float *thr = reinterpret_cast<float *>(qc_s + EX_Q);   // [128] current K'-th smallest bound (+inf until the list is full)
    int *cnt = reinterpret_cast<int *>(thr + EX_Q);        // [128]
    float *ld_ = reinterpret_cast<float *>(cnt + EX_Q);    // [128][K']
    int *li_ = reinterpret_cast<int *>(ld_ + EX_Q * a.kp); // [128][K']

    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int K = a.kp;
    const long long q0 = (long long)blockIdx.x * EX_Q;
    const int chunk = blockIdx.y;
    const int r_begin = chunk * a.rows_per_chunk;
    const int r_end = r_begin + a.rows_per_chunk < ix.n_slots ? r_begin + a.rows_per_chunk : ix.n_slots;
    if (tid < EX_Q) {
        qc_s[tid] = a.qc[q0 + tid];
        if constexpr (SELF)
            thr[tid] = a.thr0;
        else
            thr[tid] = __builtin_inff();
        cnt[tid] = 0;
    }
    __syncthreads();
    const int ld = ix.ld;
    const int nk = (ld + EX_KC - 1) / EX_KC;
    const int srow = tid >> 3, skq = tid & 7; // staging: 8 threads x float4 = 128 contiguous bytes of one row
    for (int rt = r_begin; rt < r_end; rt += EX_R) {
        f32x16 acc[4];
#pragma unroll
        for (int t = 0; t < 4; t++)
#pragma unroll
            for (int i = 0; i < 16; i++)
                acc[t][i] = 0.0f;
        float4 pa[4], pb[4];
        auto prefetch = [&](int kc) {
            const int kcol = kc * EX_KC + 4 * skq;
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const int row = srow + 32 * j;
                const bool kin = kcol < ld;
                bool qin = kin;
                if constexpr (SELF)
                    qin = kin && q0 + row < a.nq;
                pa[j] = qin ? *reinterpret_cast<const float4 *>(a.q + (size_t)(q0 + row) * ld + kcol) : make_float4(0, 0, 0, 0);
                pb[j] = (kin && rt + row < ix.n_slots)
                            ? *reinterpret_cast<const float4 *>(ix.vectors + (size_t)(rt + row) * ld + kcol)
                            : make_float4(0, 0, 0, 0);
            }
        };
        prefetch(0);
        for (int kc = 0; kc < nk; kc++) {
            __syncthreads(); // the previous stage has been consumed
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const int row = srow + 32 * j;
                float *ap = As + (4 * skq) * EX_LD + row, *bp = Bs + (4 * skq) * EX_LD + row;
                ap[0] = pa[j].x; ap[EX_LD] = pa[j].y; ap[2 * EX_LD] = pa[j].z; ap[3 * EX_LD] = pa[j].w;
                bp[0] = pb[j].x; bp[EX_LD] = pb[j].y; bp[2 * EX_LD] = pb[j].z; bp[3 * EX_LD] = pb[j].w;
            }
            __syncthreads();
            if (kc + 1 < nk)
                prefetch(kc + 1);
            const float *ar = As + (lane >> 5) * EX_LD + 32 * w + (lane & 31);
            const float *br = Bs + (lane >> 5) * EX_LD + (lane & 31);
#pragma unroll
            for (int kk = 0; kk < EX_KC / 2; kk++) {
                const float av = ar[2 * kk * EX_LD];
#pragma unroll
                for (int t = 0; t < 4; t++)
                    acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, br[2 * kk * EX_LD + 32 * t], acc[t], 0, 0, 0);
            }
        }
        // ── epilogue: bounds, threshold filter, insertion (this wavefront's 32 queries only) ──
#pragma unroll
        for (int t = 0; t < 4; t++) {
            const int row = rt + 32 * t + (lane & 31);
            const bool rv = row < r_end && ex_row_ok(ix, a.allow, row);
            const float2 xc = row < r_end ? a.xc[row] : make_float2(0.0f, 0.0f);
#pragma unroll
            for (int reg = 0; reg < 16; reg++) {
                const int ql = 32 * w + (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5); // C/D map: row of the tile = query
                const float d = ex_lower_bound<METRIC>(acc[t][reg], qc_s[ql], xc, a.uc, a.fl2);
                bool other = true;
                if constexpr (SELF)
                    other = row != a.s0 + (int)q0 + ql;
                unsigned long long m = __ballot(rv && other && q0 + ql < a.nq && d < thr[ql]);
                while (m) {
                    const int b = __ffsll((long long)m) - 1;
                    m &= m - 1;
                    const float nd = __shfl(d, b);
                    const int nrow = rt + 32 * t + (b & 31);
                    const int q = 32 * w + (reg & 3) + 8 * (reg >> 2) + 4 * (b >> 5);
                    if (!(nd < thr[q]))
                        continue;
                    const int c = cnt[q];
                    float cd = __builtin_inff();
                    int ci = -1;
                    if (lane < c) {
                        cd = ld_[q * K + lane];
                        ci = li_[q * K + lane];
                    }
                    const int pos = __popcll(__ballot(lane < c && cd <= nd));
                    __builtin_amdgcn_wave_barrier();
                    if (lane >= pos && lane < c && lane + 1 < K) {
                        ld_[q * K + lane + 1] = cd;
                        li_[q * K + lane + 1] = ci;
                    }
                    if (lane == 0) {
                        ld_[q * K + pos] = nd;
                        li_[q * K + pos] = nrow;
                        cnt[q] = c < K ? c + 1 : K;
                    }
                    __builtin_amdgcn_wave_barrier();
                    if (c + 1 >= K && lane == 0)
                        thr[q] = ld_[q * K + K - 1];
                    __builtin_amdgcn_wave_barrier();
                }
            }
        }
    }
    __builtin_amdgcn_wave_barrier();
    for (int i = 0; i < 32; i++) { // partial lists of this wavefront's queries
        const int ql = 32 * w + i;
        if (q0 + ql >= a.nq)
            break;
        const size_t o = ((size_t)chunk * a.nq + (q0 + ql));
        if (lane < K) {
            a.pd[o * K + lane] = ld_[ql * K + lane];
            a.pi[o * K + lane] = li_[ql * K + lane];
        }
        if (lane == 0)
            a.pc[o] = cnt[ql];
    }
}

// ───────────────────────── k_exact_rescore ─────────────────────────
// blockDim.x / 64 wavefronts, one query each; LDS: one padded query per wavefront.
// SELF: query q is slot a.s0 + q, read from the row store.  A deleted slot answers count -1.  The sorted list is cut at the first
// entry that fails d <= r; a full list that the cut leaves short of k cannot be certified (rows outside it have d >= cut, and
// cut <= r: one of them may lie within the radius), so it is marked.
template <int ORDER, int NCH, bool SELF = false>
__global__ void __launch_bounds__(256) k_exact_rescore(MnDevIndex ix, typename ExArgs<SELF>::type a) {
    extern __shared__ __align__(16) unsigned char smem[];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const long long q = (long long)blockIdx.x * (blockDim.x >> 6) + wv;
    bool live = q < a.nq;
    bool dead = false;
    if constexpr (SELF) {
        dead = live && ix.deleted[a.s0 + q];
        live = live && !dead;
    }
    const int K = a.kp;
    float *qs = reinterpret_cast<float *>(smem) + (size_t)wv * ix.ld;
    // lane i holds entry i of the list: the chunks' lists (each ascending) folded in row order
    float md = __builtin_inff();
    int ms = -1, c = 0;
    if (live) {
        for (int i = lane; i < ix.ld; i += 64)
            qs[i] = a.q[(size_t)q * ix.ld + i];
        for (int ch = 0; ch < a.n_chunks; ch++) {
            const size_t o = (size_t)ch * a.nq + q;
            const int pc = a.pc[o];
            float cd = __builtin_inff();
            int ci = -1;
            if (lane < pc) {
                cd = a.pd[o * K + lane];
                ci = a.pi[o * K + lane];
            }
            for (int j = 0; j < pc; j++) {
                const float nd = __shfl(cd, j);
                const int ni = __shfl(ci, j);
                if (c == K && !(nd < __shfl(md, K - 1)))
                    break;
                const int pos = __popcll(__ballot(lane < c && md <= nd));
                const float ud = __shfl_up(md, 1);
                const int us = __shfl_up(ms, 1);
                if (lane > pos && lane <= c && lane < K) {
                    md = ud;
                    ms = us;
                }
                if (lane == pos) {
                    md = nd;
                    ms = ni;
                }
                if (c < K)
                    c++;
            }
        }
    }
    __syncthreads();
    if constexpr (SELF) {
        if (dead) {
            for (int i = lane; i < a.k; i += 64) {
                a.out_ids[q * a.k + i] = -1;
                a.out_d[q * a.k + i] = __builtin_inff();
            }
            if (lane == 0)
                a.out_cnt[q] = -1;
        }
    }
    if (!live)
        return;
    const int n = c;
    const float cut = n == K ? __shfl(md, K - 1) : __builtin_inff(); // fewer than K' entries: the list holds every live row
    const float qnorm = ix.metric == 1 ? lds_self_norm<ORDER>(qs, ix.dim, ix.ld, lane) : 0.0f;
    const int myslot = lane < n ? ms : 0;
    const float d = rows_distance<ORDER, NCH>(ix, qs, qnorm, myslot, n, lane);
    const int viol = __popcll(__ballot(lane < n && d < md));
    int rank = 0;
    for (int j = 0; j < n; j++) {
        const float dj = __shfl(d, j);
        const int sj = __shfl(ms, j);
        rank += (dj < d || (dj == d && sj < ms)) ? 1 : 0;
    }
    const int k = a.k;
    int found = n < k ? n : k;
    bool keep = lane < n && rank < k;
    if constexpr (SELF) {
        const int within = __popcll(__ballot(lane < n && d <= a.r)); // ascending order: the entries within the radius come first
        found = within < k ? within : k;
        keep = keep && d <= a.r;
    }
    if (keep) {
        a.out_ids[q * k + rank] = ix.ids[ms];
        a.out_d[q * k + rank] = d;
    }
    for (int i = found + lane; i < k; i += 64) {
        a.out_ids[q * k + i] = -1;
        a.out_d[q * k + i] = __builtin_inff();
    }
    bool final_ = n < K;
    if (!final_) { // n == K' >= k
        const unsigned long long who = __ballot(lane < n && rank == k - 1);
        final_ = who != 0 && __shfl(d, __ffsll((long long)who) - 1) < cut;
        if constexpr (SELF)
            final_ = final_ && found == k;
    }
    if (lane == 0) {
        a.out_cnt[q] = found;
        atomicAdd(&a.ctr[1], (unsigned long long)n);
        if (viol)
            atomicAdd(&a.ctr[2], (unsigned long long)viol);
        if (!final_)
            a.marked[atomicAdd(&a.ctr[0], 1ull)] = (int)q;
    }
}

// ───────────────────────── k_exact_valu ─────────────────────────
// k_bruteforce's shape (mn_brute.hip): one 256-thread workgroup per query, 4 wavefronts stride over the rows 64 at a time, each
// keeping a sorted top-k in LDS (equal distances: the lower slot stays first — a wavefront meets its rows in slot order), wave 0
// merges by (d, slot).  qsel: the queries to answer (null: all nq).
// SELF (SF = ExSelf): `queries` is the row store from slot sf.s0 on, stride ld; query qi is slot sf.s0 + qi, which is never
// admitted, nor is a row with d > sf.r (so the merge ends at the cut); a deleted query slot answers count -1.
template <int ORDER, int NCH, class SF = ExNoSelf>
__global__ void __launch_bounds__(256) k_exact_valu(MnDevIndex ix, const float *queries, const int *qsel, int k, const unsigned *allow,
                                                    long long *out_ids, float *out_d, int *out_cnt, SF sf) {
    constexpr bool SELF = std::is_same<SF, ExSelf>::value;
    extern __shared__ __align__(16) unsigned char smem[];
    __shared__ int wcnt[4];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const long long qi = qsel ? qsel[blockIdx.x] : blockIdx.x;
    float *q = reinterpret_cast<float *>(smem);                 // [ld]
    float *topd = q + ix.ld;                                    // [4][EX_KMAX]
    int *tops = reinterpret_cast<int *>(topd + 4 * EX_KMAX);    // [4][EX_KMAX]
    int self = -1;
    if constexpr (SELF) {
        self = sf.s0 + (int)qi;
        if (ix.deleted[self]) { // (uniform over the workgroup)
            for (int i = tid; i < k; i += 256) {
                out_ids[qi * k + i] = -1;
                out_d[qi * k + i] = __builtin_inff();
            }
            if (tid == 0)
                out_cnt[qi] = -1;
            return;
        }
    }
    const float *qsrc = queries + (size_t)qi * (SELF ? ix.ld : ix.dim);
    for (int i = tid; i < ix.ld; i += 256)
        q[i] = (SELF || i < ix.dim) ? qsrc[i] : 0.0f;
    __syncthreads();
    float qnorm = 0.0f;
    if (ix.metric == 1)
        qnorm = lds_self_norm<ORDER>(q, ix.dim, ix.ld, lane);
    float *myd = topd + wv * EX_KMAX;
    int *mys = tops + wv * EX_KMAX;
    int cnt = 0; // wave-uniform
    for (int base = wv * 64; base < ix.n_slots; base += 256) {
        const int n = ix.n_slots - base < 64 ? ix.n_slots - base : 64;
        MnDevIndex sub = ix;
        sub.vectors = ix.vectors + (size_t)base * ix.ld;
        sub.norms = ix.norms ? ix.norms + base : nullptr;
        const int myslot = lane < n ? lane : 0;
        const float d = rows_distance<ORDER, NCH>(sub, q, qnorm, myslot, n, lane);
        bool ok = lane < n && ex_row_ok(ix, allow, base + myslot);
        if constexpr (SELF)
            ok = ok && base + myslot != self && d <= sf.r;
        const float worst = cnt >= k ? myd[k - 1] : __builtin_inff();
        unsigned long long m = __ballot(ok && (cnt < k || d < worst));
        while (m) {
            const int i = __ffsll((long long)m) - 1;
            m &= m - 1;
            const float di = __shfl(d, i);
            const int si = base + i;
            if (cnt >= k && !(di < myd[k - 1]))
                continue;
            int pos = cnt < k ? cnt : k - 1;
            __builtin_amdgcn_wave_barrier();
            if (lane == 0) {
                while (pos > 0 && (myd[pos - 1] > di)) {
                    myd[pos] = myd[pos - 1];
                    mys[pos] = mys[pos - 1];
                    pos--;
                }
                myd[pos] = di;
                mys[pos] = si;
            }
            __builtin_amdgcn_wave_barrier();
            if (cnt < k)
                cnt++;
        }
    }
    if (lane == 0)
        wcnt[wv] = cnt;
    __syncthreads();
    if (tid == 0) {
        int p[4] = {0, 0, 0, 0}, found = 0;
        for (int o = 0; o < k; o++) {
            int bw = -1;
            for (int w2 = 0; w2 < 4; w2++) {
                if (p[w2] >= wcnt[w2])
                    continue;
                const float dd = topd[w2 * EX_KMAX + p[w2]];
                const int ss = tops[w2 * EX_KMAX + p[w2]];
                if (bw < 0 || dd < topd[bw * EX_KMAX + p[bw]] ||
                    (dd == topd[bw * EX_KMAX + p[bw]] && ss < tops[bw * EX_KMAX + p[bw]]))
                    bw = w2;
            }
            if (bw < 0) {
                out_ids[qi * k + o] = -1;
                out_d[qi * k + o] = __builtin_inff();
            } else {
                out_ids[qi * k + o] = ix.ids[tops[bw * EX_KMAX + p[bw]]];
                out_d[qi * k + o] = topd[bw * EX_KMAX + p[bw]];
                p[bw]++;
                found++;
            }
        }
        out_cnt[qi] = found;
    }
}

// an index without slots: every answer is empty
__global__ void k_exact_fill(long long nq, int k, long long *out_ids, float *out_d, int *out_cnt) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < nq * k) {
        out_ids[i] = -1;
        out_d[i] = __builtin_inff();
    }
    if (i < nq)
        out_cnt[i] = 0;
}

// ───────────────────────── host side ─────────────────────────
void mn_launch_exact_fill(long long nq, int k, long long *d_out_ids, float *d_out_d, int *d_out_cnt, hipStream_t st) {
    const long long n = nq * k > nq ? nq * k : nq;
    hipLaunchKernelGGL(k_exact_fill, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, nq, k, d_out_ids, d_out_d, d_out_cnt);
}

size_t mn_exact_valu_lds_bytes(int ld) { return (size_t)ld * sizeof(float) + 4 * EX_KMAX * (sizeof(float) + sizeof(int)); }

// the index's inner loop over every row for queries d_qsel[0..n) (null: 0..n-1); the self-join's queries are the rows from slot s0
int mn_launch_exact_valu(const MnDevIndex &ix, const float *d_queries, const int *d_qsel, long long n, int k, const unsigned *d_allow,
                         long long *d_out_ids, float *d_out_d, int *d_out_cnt, const MnExactSelf *self, hipStream_t st) {
    if (n <= 0)
        return 0;
    if (k <= 0 || k > EX_KMAX || (self && (self->s0 < 0 || self->s0 >= ix.n_slots || self->r != self->r)))
        return -1;
    const size_t lds = mn_exact_valu_lds_bytes(ix.ld);
    const dim3 grid((unsigned)n), block(256);
    mn_for_row_walk(ix.order, ix.ld, [&](auto O, auto N) {
        if (self) {
            ExSelf sf;
            sf.s0 = self->s0;
            sf.r = self->r;
            hipLaunchKernelGGL((k_exact_valu<O(), N(), ExSelf>), grid, block, lds, st, ix, ix.vectors + (size_t)self->s0 * ix.ld, d_qsel,
                               k, (const unsigned *)nullptr, d_out_ids, d_out_d, d_out_cnt, sf);
        } else {
            hipLaunchKernelGGL((k_exact_valu<O(), N()>), grid, block, lds, st, ix, d_queries, d_qsel, k, d_allow, d_out_ids, d_out_d,
                               d_out_cnt, ExNoSelf());
        }
    });
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

// One candidate pass's scratch, as byte offsets: the padded queries and their constants (zeroed together), the rows' constants, the
// row chunks' partial lists.  The self-join reads its queries from the row store and brings the rows' constants along
// (mn_launch_knn_prep_rows): its qpad and xc parts are empty.
struct ExLayout {
    int n_chunks, rows_per_chunk;
    long long q_tiles;
    size_t qpad, qc, xc, pd, pi, pc, total;
};
// row chunks as mn_brute_mfma_scratch_bytes cuts them
static void ex_chunks(const MnDevIndex &ix, long long nq, int *n_chunks, int *rows_per_chunk) {
    const long long qt = (nq + EX_Q - 1) / EX_Q;
    long long want = (1024 + qt - 1) / qt;
    const long long max_chunks = (ix.n_slots + 8 * EX_R - 1) / (8 * EX_R);
    if (want > max_chunks)
        want = max_chunks;
    if (want < 1)
        want = 1;
    int rpc = (int)((ix.n_slots + want - 1) / want);
    rpc = (rpc + EX_R - 1) / EX_R * EX_R;
    *n_chunks = (ix.n_slots + rpc - 1) / rpc;
    *rows_per_chunk = rpc;
}
static ExLayout ex_layout(const MnDevIndex &ix, long long nq, int kp, bool self) {
    ExLayout L;
    L.q_tiles = (nq + EX_Q - 1) / EX_Q;
    ex_chunks(ix, nq, &L.n_chunks, &L.rows_per_chunk);
    auto up = [](size_t b) { return (b + 255) & ~(size_t)255; };
    const size_t nq_pad = (size_t)L.q_tiles * EX_Q, list = up((size_t)L.n_chunks * nq * kp * 4);
    L.qpad = 0;
    L.qc = L.qpad + (self ? 0 : up(nq_pad * ix.ld * 4));
    L.xc = L.qc + up(nq_pad * 8);
    L.pd = L.xc + (self ? 0 : up((size_t)ix.n_slots * 8));
    L.pi = L.pd + list;
    L.pc = L.pi + list;
    L.total = L.pc + up((size_t)L.n_chunks * nq * 4);
    return L;
}

size_t mn_exact_mfma_scratch_bytes(const MnDevIndex &ix, long long nq, int kp, bool self) { return ex_layout(ix, nq, kp, self).total; }

static void ex_bound_consts(int ld, float *uc, float *fl2) {
    // what gradual underflow can lose of either dot product (2^-150 per operation), with room to spare
    *uc = (float)(ld + 8) * 0x1p-140f;
    const double nu = (double)(ld + 8) * 0x1p-24, g = nu / (1.0 - nu);
    float f = (float)(1.0 - 4.0 * g - 0x1p-20);
    while ((double)f > 1.0 - 4.0 * g - 0x1p-20)
        f = nextafterf(f, 0.0f);
    *fl2 = f;
}

template <bool SELF>
static int launch_exact_mfma(const MnDevIndex &ix, const float *d_queries, long long nq, int k, int kp, const unsigned *d_allow,
                             void *scratch, long long *d_out_ids, float *d_out_d, int *d_out_cnt, unsigned long long *d_ctr,
                             int *d_marked, const MnExactSelf *self, hipStream_t st) {
    const size_t lds = ex_mfma_lds_bytes(kp);
    const bool granted = ix.metric == 1   ? mn_lds_grant_for(k_exact_mfma<1, SELF>, lds)
                         : ix.metric == 0 ? mn_lds_grant_for(k_exact_mfma<0, SELF>, lds)
                                          : mn_lds_grant_for(k_exact_mfma<2, SELF>, lds);
    if (!granted)
        return 1;
    typename ExArgs<SELF>::type a;
    const ExLayout L = ex_layout(ix, nq, kp, SELF);
    a.n_chunks = L.n_chunks;
    a.rows_per_chunk = L.rows_per_chunk;
    unsigned char *p = static_cast<unsigned char *>(scratch);
    float *qpad = SELF ? nullptr : reinterpret_cast<float *>(p + L.qpad);
    float2 *qc = reinterpret_cast<float2 *>(p + L.qc);
    a.pd = reinterpret_cast<float *>(p + L.pd);
    a.pi = reinterpret_cast<int *>(p + L.pi);
    a.pc = reinterpret_cast<int *>(p + L.pc);
    // the padding queries of the last tile: zero rows, zero constants (their columns of the tile are never looked at; the
    // self-join's are neither read nor looked at)
    if (hipMemsetAsync(p + L.qpad, 0, L.xc - L.qpad, st) != hipSuccess)
        return -1;
    const float *rows = d_queries;
    if constexpr (SELF)
        rows = ix.vectors + (size_t)self->s0 * ix.ld;
    const size_t qlds = (size_t)ix.ld * 4;
    if (ix.order == MN_ORDER_SSE_V)
        hipLaunchKernelGGL((k_exact_prep_q<MN_ORDER_SSE_V, SELF>), dim3((unsigned)nq), dim3(64), qlds, st, ix, rows, nq, qpad, qc);
    else
        hipLaunchKernelGGL((k_exact_prep_q<MN_ORDER_WAVE_V, SELF>), dim3((unsigned)nq), dim3(64), qlds, st, ix, rows, nq, qpad, qc);
    if constexpr (SELF) {
        a.q = rows;
        a.xc = static_cast<const float2 *>(self->d_xc);
        a.s0 = self->s0;
        a.r = self->r;
        a.thr0 = nextafterf(self->r, __builtin_inff()); // lb < thr0 is lb <= r (r = +inf stays +inf)
    } else {
        mn_launch_knn_prep_rows(ix, p + L.xc, st);
        a.q = qpad;
        a.xc = reinterpret_cast<const float2 *>(p + L.xc);
    }
    a.qc = qc;
    a.allow = d_allow;
    a.nq = nq;
    a.k = k;
    a.kp = kp;
    ex_bound_consts(ix.ld, &a.uc, &a.fl2);
    a.out_ids = d_out_ids;
    a.out_d = d_out_d;
    a.out_cnt = d_out_cnt;
    a.ctr = d_ctr;
    a.marked = d_marked;
    const dim3 grid((unsigned)L.q_tiles, (unsigned)a.n_chunks);
    if (ix.metric == 1)
        hipLaunchKernelGGL((k_exact_mfma<1, SELF>), grid, dim3(256), lds, st, ix, a);
    else if (ix.metric == 0)
        hipLaunchKernelGGL((k_exact_mfma<0, SELF>), grid, dim3(256), lds, st, ix, a);
    else
        hipLaunchKernelGGL((k_exact_mfma<2, SELF>), grid, dim3(256), lds, st, ix, a);
    // re-score: 4 queries per workgroup while their padded copies fit 32 KB of LDS, else one
    const int wpb = (size_t)ix.ld * 16 <= 32 * 1024 ? 4 : 1;
    const dim3 rgrid((unsigned)((nq + wpb - 1) / wpb)), rblock(64 * wpb);
    const size_t rlds = (size_t)ix.ld * 4 * wpb;
    mn_for_row_walk(ix.order, ix.ld, [&](auto O, auto N) {
        hipLaunchKernelGGL((k_exact_rescore<O(), N(), SELF>), rgrid, rblock, rlds, st, ix, a);
    });
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

// the rows' constants of the bound: the search computes them per call into its scratch, the self-join once for all its batches
void mn_launch_knn_prep_rows(const MnDevIndex &ix, void *d_xc, hipStream_t st) {
    hipLaunchKernelGGL(k_exact_prep_rows, dim3((unsigned)(((long long)ix.n_slots * 16 + 255) / 256)), dim3(256), 0, st, ix,
                       static_cast<float2 *>(d_xc));
}

// Candidate pass + re-score + certificate for all nq queries, or for the query slots [s0, s0 + nq) of the self-join.  d_ctr [3] must be
// zero on entry; d_marked [nq].  1: the device does not grant the LDS the lists need (nothing was launched: the caller takes
// k_exact_valu); 0 / -1.
int mn_launch_exact_mfma(const MnDevIndex &ix, const float *d_queries, long long nq, int k, int kp, const unsigned *d_allow,
                         void *scratch, long long *d_out_ids, float *d_out_d, int *d_out_cnt, unsigned long long *d_ctr,
                         int *d_marked, const MnExactSelf *self, hipStream_t st) {
    if (nq <= 0 || k <= 0 || kp < k || kp > 64 || ix.n_slots <= 0)
        return -1;
    if (!self)
        return launch_exact_mfma<false>(ix, d_queries, nq, k, kp, d_allow, scratch, d_out_ids, d_out_d, d_out_cnt, d_ctr, d_marked,
                                        nullptr, st);
    if (self->s0 < 0 || self->s0 + nq > ix.n_slots || self->r != self->r)
        return -1;
    return launch_exact_mfma<true>(ix, nullptr, nq, k, kp, nullptr, scratch, d_out_ids, d_out_d, d_out_cnt, d_ctr, d_marked, self, st);
}
