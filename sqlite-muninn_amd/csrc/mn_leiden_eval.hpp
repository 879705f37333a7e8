// mn_leiden_eval.hpp — what a wavefront does to evaluate ONE node of a Leiden sweep (the loop body of
// src/graph_community.c:158-216): device code only, nothing here launches or allocates.  Included by mn_leiden.hip alone
// (device code does not cross a translation unit); its kernels decide which nodes are evaluated by which of these.
//
// All arithmetic is f64 and every per-community sum is taken in adjacency-list order, as the reference's.  Three evaluations,
// the same decisions bit for bit:
//   best_move          one wavefront, one node: the edges' (community, weight, eligible) triples are staged in list order — LDS
//                      up to LEI_CAP edges, global scratch above —, lane e decides whether edge e is the first occurrence of
//                      its community and sums that community's weights in list order; a max-with-lowest-index reduction
//                      reproduces the strict `gain > best_gain` first-seen rule (:212).  The sequential kernel's evaluation
//                      (COH: agent-scope loads, never a stale line), and that of nodes past LEI_CAP edges otherwise.
//   best_move_hash     unweighted graphs: counts in a small open-addressing table in LDS keyed by community
//   best_move_wslots   weighted graphs: the same table numbers the communities, a lane per community sums in list order
// The last two serve SG-lane sub-groups (64 / SG nodes per wavefront, nodes of at most LEI_SG_CAP edges) and whole wavefronts
// (SG = 64, wide nodes) alike and share lei_head, lei_table_slot, lei_gain and LeiBest; the three four-in-flight edge loaders
// differ in clamping, weights and padding and are written out.  LeiArgs is the argument block of every Leiden kernel.
#pragma once
#include "mn_graph_int.hpp"

#define LEI_CAP 1024 // edges of one node staged in LDS; larger nodes use the global scratch path
#ifndef LEI_SG_CAP
#define LEI_SG_CAP 64 // sub-group evaluation: edges staged per node (more → the node takes a whole wavefront); power of two
#endif
// ints per sub-group: table of 1 << log2h entries (key, count, first position) + counter (4 ints) + 16-bit slot list (one per
// edge at most).  log2h is LEI_SG_LOG2H (two entries per edge) while most labels are still different — the first sweeps of a
// phase — and one less afterwards (round 4): the table then takes half the LDS and 32 wavefronts fit a CU instead of 20.  Only
// communities other than the node's own enter it, at most one per edge, so it cannot overflow at either size.
#define LEI_SG_AREA_OF(log2h) (3 * (1 << (log2h)) + 4 + LEI_SG_CAP / 2)
#define LEI_SG_LOG2H (LEI_SG_CAP == 32 ? 6 : LEI_SG_CAP == 64 ? 7 : LEI_SG_CAP == 128 ? 8 : 9) // table of 2 * LEI_SG_CAP entries
#define LEI_EMPTY (-1)   // a free table entry
#define LEI_FX 1048576.0 // fixed point (2^20) of the movers' degree tallies

// a load the sequential kernel (COH) takes at agent scope: labels and sums change under it
template <bool COH> DEVI int ld_i(const int *p) { return COH ? __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : *p; }
template <bool COH> DEVI double ld_d(const double *p) { return COH ? __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : *p; }

// gain of moving a node of degree k_v from its community (total st_old, the node's weight into it k_v_to_old) to one of
// total st_c that the node has weight sacc into: the expression of :209-210, verbatim
DEVI double lei_gain(double sacc, double k_v_to_old, double m, double resolution, double k_v, double st_old, double st_c) {
    return (sacc - k_v_to_old) / m + resolution * k_v * (st_old - k_v - st_c) / (2.0 * m * m);
}

// Returns the community node v should move to (== its current one if no strictly positive gain).
// ec/ew/el: staging for the node's edges (community, weight, eligible) in list order — LDS for degree
// <= LEI_CAP, global scratch otherwise; both 16-byte aligned, capacity rounded up to a multiple of 4.
template <bool COH>
DEVI int best_move(const DevGraph &g, int v, const int *label, const double *sum_tot, const double *kdeg, double m,
                   double resolution, int use_both, const int *elig_part, int *ec, double *ew, unsigned char *el, int lane,
                   double *dk_out = nullptr, int pickless = 0) {
    const int o0 = g.off_out[v], d_out = g.off_out[v + 1] - o0;
    const int i0 = use_both ? g.off_in[v] : 0, d_in = use_both ? g.off_in[v + 1] - i0 : 0;
    const int d = d_out + d_in;
    const int d4 = (d + 3) & ~3;
    const int old = ld_i<COH>(label + v);
    const int mypart = elig_part ? elig_part[v] : 0;
    __builtin_amdgcn_wave_barrier();
    if (COH) {
        for (int e = lane; e < d4; e += 64) {
            int c = -2; // padding never matches a community
            double w = 0.0;
            unsigned char ok = 0;
            if (e < d) {
                int t;
                if (e < d_out) {
                    t = g.tgt_out[o0 + e];
                    w = g.w_out ? g.w_out[o0 + e] : 1.0;
                } else {
                    t = g.tgt_in[i0 + (e - d_out)];
                    w = g.w_in ? g.w_in[i0 + (e - d_out)] : 1.0;
                }
                c = ld_i<COH>(label + t);
                ok = (!elig_part || elig_part[t] == mypart) ? 1 : 0;
            }
            ec[e] = c;
            ew[e] = w;
            el[e] = ok;
        }
    } else {
        // parallel rounds: four edges per lane in flight — every load unconditional (index clamped to the last edge), the four
        // targets and weights go out back to back, then the four labels (and partitions): two round trips per 256 edges
        // instead of two per 64 (the guarded one-edge-per-lane loop above is one s_waitcnt per load)
        const bool has_w = g.w_out != nullptr || g.w_in != nullptr;
        for (int e0 = 0; e0 < d4; e0 += 256) {
            int t[4], c[4], part[4];
            double w[4];
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const int ecl = max(0, min(e0 + j * 64 + lane, d - 1));
                const bool out = ecl < d_out;
                t[j] = *(out ? g.tgt_out + o0 + ecl : g.tgt_in + i0 + (ecl - d_out));
                w[j] = 1.0;
                if (has_w) {
                    const double *pw = out ? g.w_out : g.w_in;
                    w[j] = pw ? pw[(out ? o0 + ecl : i0 + (ecl - d_out))] : 1.0;
                }
            }
#pragma unroll
            for (int j = 0; j < 4; j++)
                c[j] = label[t[j]];
            if (elig_part) {
#pragma unroll
                for (int j = 0; j < 4; j++)
                    part[j] = elig_part[t[j]];
            }
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const int e = e0 + j * 64 + lane;
                if (e >= d4)
                    continue;
                const bool in = e < d;
                ec[e] = in ? c[j] : -2;
                ew[e] = in ? w[j] : 0.0;
                el[e] = in && (!elig_part || part[j] == mypart) ? 1 : 0;
            }
        }
    }
    __builtin_amdgcn_s_waitcnt(0);
    __builtin_amdgcn_wave_barrier();
    const double k_v = kdeg[v];
    const int4 *ec4 = reinterpret_cast<const int4 *>(ec);
    const double2 *ew2 = reinterpret_cast<const double2 *>(ew);
    const uchar4 *el4 = reinterpret_cast<const uchar4 *>(el);
    double k_v_to_old = 0.0; // weight_to_community(v, old), :163 — list order
    for (int q = 0; q < (d4 >> 2); q++) {
        const int4 cj = ec4[q];
        const double2 wa = ew2[2 * q], wb = ew2[2 * q + 1];
        if (cj.x == old) k_v_to_old += wa.x;
        if (cj.y == old) k_v_to_old += wa.y;
        if (cj.z == old) k_v_to_old += wb.x;
        if (cj.w == old) k_v_to_old += wb.y;
    }
    const double st_old = ld_d<COH>(sum_tot + old);
    double best_gain = 0.0;
    int best = old;
    for (int base = 0; base < d; base += 64) {
        const int e = base + lane;
        const int c = e < d ? ec[e] : -3;
        bool cand = e < d && el[e] && c != old && !(pickless && c > old);
        // one pass over the list: the in-order weight sum of community c (weight_to_community, :206) and
        // "an eligible earlier edge already carries c" (the dedup scan of :173-199)
        double sacc = 0.0;
        bool dup = false;
        for (int q = 0; q < (d4 >> 2); q++) {
            const int4 cj = ec4[q];
            const double2 wa = ew2[2 * q], wb = ew2[2 * q + 1];
            const uchar4 ej = el4[q];
            const int j = q << 2;
            if (cj.x == c) { sacc += wa.x; dup |= (j < e) && ej.x; }
            if (cj.y == c) { sacc += wa.y; dup |= (j + 1 < e) && ej.y; }
            if (cj.z == c) { sacc += wb.x; dup |= (j + 2 < e) && ej.z; }
            if (cj.w == c) { sacc += wb.y; dup |= (j + 3 < e) && ej.w; }
        }
        cand = cand && !dup;
        double gain = -1.0, dk = 0.0;
        if (cand) {
            const double st_c = ld_d<COH>(sum_tot + c);
            dk = sacc - k_v_to_old;
            gain = lei_gain(sacc, k_v_to_old, m, resolution, k_v, st_old, st_c);
            if (!(gain > 0.0))
                gain = -1.0; // also drops NaN: `gain > best_gain` is false for it
        }
        // max gain, lowest lane on ties == first candidate with the strictly largest gain
        double bg = gain;
        int bl = lane;
        for (int mk = 32; mk >= 1; mk >>= 1) {
            double og = __shfl_xor(bg, mk);
            int ol = __shfl_xor(bl, mk);
            if (og > bg || (og == bg && ol < bl)) {
                bg = og;
                bl = ol;
            }
        }
        if (bg > best_gain) { // strict: an equal gain in a later chunk does not replace (:212)
            best_gain = bg;
            best = __shfl(c, bl);
            double bdk = __shfl(dk, bl);
            if (dk_out)
                *dk_out = bdk;
        }
    }
    return best;
}

// ── the table evaluations: what best_move_hash and best_move_wslots share ──

// everything about node v whose address depends on v alone: requested together, one round trip
struct LeiHead {
    int o0, d_out, i0, d_in, old, mypart;
    double k_v;
};
DEVI LeiHead lei_head(const DevGraph &g, int v, const int *label, const double *kdeg, int use_both, const int *elig_part) {
    LeiHead h;
    const int o0 = g.off_out[v], o1 = g.off_out[v + 1];
    const int i0 = g.off_in[use_both ? v : 0], i1 = g.off_in[use_both ? v + 1 : 0]; // (unconditional loads)
    h.old = label[v];
    h.mypart = (elig_part ? elig_part : label)[v];
    h.k_v = kdeg[v];
    h.o0 = o0;
    h.d_out = o1 - o0;
    h.i0 = use_both ? i0 : 0;
    h.d_in = use_both ? i1 - i0 : 0;
    return h;
}

DEVI unsigned lei_hash(int c, int log2h) { return ((unsigned)c * 2654435761u) >> (32 - log2h); }

// The slot of community c in the open-addressing table tk (H = 1 << log2h keys, LEI_EMPTY = free), inserting it if it is not
// there; whoever inserts a key runs init(slot) — LDS operations of one wavefront execute in program order, so what init
// stores is in place before anyone's additions, which come after the probe loop.
template <typename F> DEVI unsigned lei_table_slot(int *tk, int H, int log2h, int c, F init) {
    unsigned h = lei_hash(c, log2h);
    for (;;) {
        int prev = tk[h]; // (a plain read first: most edges find their community already inserted)
        if (prev == LEI_EMPTY) {
            prev = atomicCAS(&tk[h], LEI_EMPTY, c);
            if (prev == LEI_EMPTY)
                init(h);
        }
        if (prev == LEI_EMPTY || prev == c)
            break;
        h = (h + 1) & (H - 1);
    }
    return h;
}

// Lane exchange for the reductions inside a sub-group, without the LDS crossbar (__shfl_xor = ds_bpermute, and the SQ counters of
// round 4 put this kernel's LDS pipe at ≈ 88 % busy): DPP inside a row of 16 lanes — quad exchanges, then the mirrors (any pairing
// that ends with every lane holding the row's result serves a commutative, associative reduction) —, shuffles only above 16.
template <int STEP> DEVI int lei_peer(int v) {
    if (STEP == 0) return __builtin_amdgcn_update_dpp(0, v, 0xB1, 0xF, 0xF, false);  // quad_perm [1,0,3,2]
    if (STEP == 1) return __builtin_amdgcn_update_dpp(0, v, 0x4E, 0xF, 0xF, false);  // quad_perm [2,3,0,1]
    if (STEP == 2) return __builtin_amdgcn_update_dpp(0, v, 0x141, 0xF, 0xF, false); // row_half_mirror
    if (STEP == 3) return __builtin_amdgcn_update_dpp(0, v, 0x140, 0xF, 0xF, false); // row_mirror
    return __shfl_xor(v, STEP == 4 ? 16 : 32);
}
template <int STEP> DEVI double lei_peer(double v) {
    return __hiloint2double(lei_peer<STEP>(__double2hiint(v)), lei_peer<STEP>(__double2loint(v)));
}
// the sum of x over the SG lanes of a sub-group, in every lane
template <int SG> DEVI int lei_sg_sum(int x) {
    x += lei_peer<0>(x);
    x += lei_peer<1>(x);
    x += lei_peer<2>(x);
    x += lei_peer<3>(x);
    if (SG > 16)
        x += lei_peer<4>(x);
    if (SG > 32)
        x += lei_peer<5>(x);
    return x;
}

// the best candidate so far: max gain, ties to the lowest first position = the strict first-seen rule (:212), in any order
struct LeiBest {
    double gain, dk;
    int pos, c;
};
DEVI void lei_best_offer(LeiBest &b, double gain, int pos, int c, double dk) {
    if (!(gain > 0.0)) // (also drops NaN)
        return;
    if (gain > b.gain || (gain == b.gain && pos < b.pos)) {
        b.gain = gain;
        b.pos = pos;
        b.c = c;
        b.dk = dk;
    }
}
template <int STEP> DEVI void lei_best_step(LeiBest &b) {
    const double og = lei_peer<STEP>(b.gain), od = lei_peer<STEP>(b.dk);
    const int op = lei_peer<STEP>(b.pos), oc = lei_peer<STEP>(b.c);
    if (og > b.gain || (og == b.gain && op < b.pos)) {
        b.gain = og;
        b.pos = op;
        b.c = oc;
        b.dk = od;
    }
}
// the sub-group's best candidate: its community (old if there is none) and, in *dk_out, its weight difference
template <int SG> DEVI int lei_best_reduce(LeiBest b, int old, double *dk_out) {
    lei_best_step<0>(b);
    lei_best_step<1>(b);
    lei_best_step<2>(b);
    lei_best_step<3>(b);
    if (SG > 16)
        lei_best_step<4>(b);
    if (SG > 32)
        lei_best_step<5>(b);
    *dk_out = b.gain > 0.0 ? b.dk : 0.0;
    return b.gain > 0.0 ? b.c : old;
}

// ── unweighted graphs: O(degree) evaluation ──
// Every weight is 1.0, so weight_to_community(v, c) (:75-90) is the NUMBER of v's edges into c — an integer, exact in
// any order — and the O(deg · #neighbour communities) rescans of the reference (and of best_move above, which keeps
// them because weighted sums must be taken in list order) collapse into one pass: each edge is dropped into a small
// open-addressing table in LDS keyed by community (count, position of the first eligible edge).  The candidates are
// the occupied entries; the strict-gain first-seen rule (:212) = highest gain, lowest first position.  Same decisions
// as best_move, bit for bit (the gain expression is evaluated on the same f64 operands).
//
// SG lanes (lane = absolute lane, sl = lane % SG) evaluate node hd; tk/tc/tp: the group's table of H = 1 << log2h entries.
// Round 4 (the kernel is bound by the LDS pipe): (i) only the KEYS are cleared, four per ds_write_b128 — whoever inserts a key
// initialises its count and position; (ii) edges into the node's own community, most of them once communities have formed,
// never touch the table: weight_to_community(v, old) is counted in registers and reduced across the sub-group by DPP; (iii) the
// closing max-reduction runs on DPP as well.  Same decisions, bit for bit.
template <int SG>
DEVI int best_move_hash(const DevGraph &g, const LeiHead &hd, const int *label, const double *sum_tot, double m,
                        double resolution, const int *elig_part, int *tk, int *tc, int *tp, int *cl, int log2h, int lane,
                        int sl, double *dk_out, int pickless) {
    const int H = 1 << log2h;
    const int o0 = hd.o0, d_out = hd.d_out, i0 = hd.i0, d_in = hd.d_in;
    const int d = d_out + d_in;
    const int old = hd.old;
    const int mypart = elig_part ? hd.mypart : 0;
    // issued now, consumed after the table is built: this round trip overlaps the targets → labels chain
    const double k_v = hd.k_v;
    const double st_old = sum_tot[old];
    for (int j = 4 * sl; j < H; j += 4 * SG)
        *reinterpret_cast<int4 *>(tk + j) = make_int4(LEI_EMPTY, LEI_EMPTY, LEI_EMPTY, LEI_EMPTY);
    // cl[0]: number of occupied entries; then their slots (16-bit), appended by whoever inserts a key — the candidate
    // scan below visits the occupied entries only (a handful once communities have formed), not the whole table
    unsigned short *clist = reinterpret_cast<unsigned short *>(cl + 4);
    if (sl == 0)
        cl[0] = 0;
    __builtin_amdgcn_wave_barrier();
    int n_old = 0; // this lane's edges into the node's own community
    // Four edges per lane at a time, every load unconditional (index clamped to the last edge): the four targets go out
    // back to back, then their four labels (and partitions) — two round trips per 4·SG edges instead of two per SG edges.
    for (int e0 = 0; e0 < d; e0 += 4 * SG) {
        int t[4], c[4], part[4];
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const int ec = min(e0 + j * SG + sl, d - 1);
            const int *pt = ec < d_out ? g.tgt_out + o0 + ec : g.tgt_in + i0 + (ec - d_out);
            t[j] = *pt;
        }
#pragma unroll
        for (int j = 0; j < 4; j++)
            c[j] = label[t[j]];
        if (elig_part) {
#pragma unroll
            for (int j = 0; j < 4; j++)
                part[j] = elig_part[t[j]];
        } else {
#pragma unroll
            for (int j = 0; j < 4; j++)
                part[j] = mypart;
        }
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const int e = e0 + j * SG + sl;
            if (e >= d)
                continue;
            if (c[j] == old) {
                n_old++;
                continue;
            }
            // refinement: a target in another phase-1 community carries a refined label that no candidate of this node can
            // have (a refined community lies inside one phase-1 community, and candidates need an eligible edge) and that is
            // not `old` either: it changes no count that is looked at — it does not enter the table
            if (part[j] != mypart)
                continue;
            const unsigned h = lei_table_slot(tk, H, log2h, c[j], [&](unsigned s) {
                tc[s] = 0;
                tp[s] = 0x7fffffff;
                clist[atomicAdd(&cl[0], 1)] = (unsigned short)s;
            });
            atomicAdd(&tc[h], 1);
            atomicMin(&tp[h], e);
        }
    }
    __builtin_amdgcn_s_waitcnt(0);
    __builtin_amdgcn_wave_barrier();
    const double k_v_to_old = (double)lei_sg_sum<SG>(n_old); // weight_to_community(v, old), :163
    LeiBest b = {-1.0, 0.0, 0x7fffffff, old};
    // candidates = the occupied entries, one per lane per pass (max gain, ties to the lowest first position: any order)
    const int ncand = cl[0];
    for (int i = sl; i < ncand; i += SG) {
        const int slot = clist[i];
        const int c = tk[slot], pos = tp[slot];
        if (pos == 0x7fffffff || (pickless && c > old))
            continue;
        const double sacc = (double)tc[slot];
        const double st_c = sum_tot[c];
        lei_best_offer(b, lei_gain(sacc, k_v_to_old, m, resolution, k_v, st_old, st_c), pos, c, sacc - k_v_to_old);
    }
    return lei_best_reduce<SG>(b, old, dk_out);
}

// ── weighted graphs: O(degree · distinct communities / lanes) evaluation (round 4) ──
// weight_to_community(v, c) (:75-90) is an f64 sum in LIST ORDER, so the hash-and-count shortcut of the unweighted path does not
// apply — but the sum does not have to be taken once per EDGE (best_move: every lane sums the community of its own edge, most of
// them the same few communities: O(degree²) compare-and-add steps, 70 % of a weighted run).  Here every edge is hashed to its
// community's table slot (as in best_move_hash; the slot remembers the first eligible position), communities are numbered in
// the order they were inserted, and lane p OWNS community number p: one walk over the staged list in order, adding the weights
// of the edges whose community number is p — the reference's additions in the reference's order, once per distinct community.
// Sixteen lanes cover sixteen communities per walk; once communities have formed a node's neighbours lie in a handful.
// Bytes of one evaluation's area for `cap` staged edges and a table of 1 << log2h entries (the layout below).
__host__ DEVI size_t lei_wslots_bytes(int cap, int log2h) { return (size_t)20 * cap + (size_t)10 * ((size_t)1 << log2h) + 16; }
template <int SG>
DEVI int best_move_wslots(const DevGraph &g, const LeiHead &hd, const int *label, const double *sum_tot, double m, double resolution,
                          const int *elig_part, unsigned char *area, int cap, int log2h, int lane, int sl, double *dk_out,
                          int pickless) {
    const int H = 1 << log2h;
    double *ew = reinterpret_cast<double *>(area);           // [cap] weights in list order (padding 0.0)
    double *ssum = ew + cap;                                  // [cap] in-order weight sum of community number p
    int *tk = reinterpret_cast<int *>(ssum + cap);            // [H] community of a slot
    int *tp = tk + H;                                         // [H] first eligible position
    unsigned short *tpos = reinterpret_cast<unsigned short *>(tp + H); // [H] slot -> community number
    unsigned short *spos = tpos + H;                          // [cap] community number -> slot
    unsigned short *es = spos + cap;                          // [cap] edge -> slot, then edge -> community number (padding 0xFFFF)
    int *cnt = reinterpret_cast<int *>(es + cap);
    const int o0 = hd.o0, d_out = hd.d_out, i0 = hd.i0, d_in = hd.d_in;
    const int d = d_out + d_in;
    const int d4 = (d + 3) & ~3;
    const int old = hd.old;
    const int mypart = elig_part ? hd.mypart : 0;
    const double k_v = hd.k_v;
    *dk_out = 0.0;
    if (d == 0)
        return old;
    const double st_old = sum_tot[old];
    for (int j = 4 * sl; j < H; j += 4 * SG)
        *reinterpret_cast<int4 *>(tk + j) = make_int4(LEI_EMPTY, LEI_EMPTY, LEI_EMPTY, LEI_EMPTY);
    if (sl == 0)
        cnt[0] = 0;
    __builtin_amdgcn_wave_barrier();
    for (int e0 = 0; e0 < d4; e0 += 4 * SG) { // four edges per lane in flight: targets + weights, then labels (+ partitions)
        int t[4], c[4], part[4];
        double w[4];
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const int ecl = min(e0 + j * SG + sl, d - 1);
            const bool out = ecl < d_out;
            t[j] = *(out ? g.tgt_out + o0 + ecl : g.tgt_in + i0 + (ecl - d_out));
            const double *pw = out ? g.w_out : g.w_in;
            w[j] = pw ? pw[out ? o0 + ecl : i0 + (ecl - d_out)] : 1.0;
        }
#pragma unroll
        for (int j = 0; j < 4; j++)
            c[j] = label[t[j]];
#pragma unroll
        for (int j = 0; j < 4; j++)
            part[j] = elig_part ? elig_part[t[j]] : mypart;
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const int e = e0 + j * SG + sl;
            if (e >= d4)
                continue;
            if (e >= d) {
                ew[e] = 0.0;
                es[e] = 0xFFFF;
                continue;
            }
            ew[e] = w[j];
            const unsigned h = lei_table_slot(tk, H, log2h, c[j], [&](unsigned s) { // (the inserter numbers the community)
                const int p = atomicAdd(&cnt[0], 1);
                tpos[s] = (unsigned short)p;
                spos[p] = (unsigned short)s;
                tp[s] = 0x7fffffff;
            });
            es[e] = (unsigned short)h;
            if (part[j] == mypart)
                atomicMin(&tp[h], e);
        }
    }
    __builtin_amdgcn_s_waitcnt(0);
    __builtin_amdgcn_wave_barrier();
    for (int e = sl; e < d; e += SG) // slot -> community number
        es[e] = tpos[es[e]];
    __builtin_amdgcn_wave_barrier();
    const int ncomm = cnt[0];
    const ushort4 *es4 = reinterpret_cast<const ushort4 *>(es);
    const double2 *ew2 = reinterpret_cast<const double2 *>(ew);
    for (int p0 = 0; p0 < ncomm; p0 += SG) { // lane p walks the list for community number p: list-order f64 sum (:75-90)
        const int p = p0 + sl;
        const unsigned short my = p < ncomm ? (unsigned short)p : (unsigned short)0xFFFE;
        double acc = 0.0;
        for (int q = 0; q < (d4 >> 2); q++) {
            const ushort4 e4 = es4[q];
            const double2 wa = ew2[2 * q], wb = ew2[2 * q + 1];
            if (e4.x == my) acc += wa.x;
            if (e4.y == my) acc += wa.y;
            if (e4.z == my) acc += wb.x;
            if (e4.w == my) acc += wb.y;
        }
        if (p < ncomm)
            ssum[p] = acc;
    }
    __builtin_amdgcn_wave_barrier();
    double k_v_to_old = 0.0; // weight_to_community(v, old), :163
    {
        unsigned h = lei_hash(old, log2h);
        for (int probe = 0; probe < H; probe++) {
            const int key = tk[h];
            if (key == old) {
                k_v_to_old = ssum[tpos[h]];
                break;
            }
            if (key == LEI_EMPTY)
                break;
            h = (h + 1) & (H - 1);
        }
    }
    LeiBest b = {-1.0, 0.0, 0x7fffffff, old};
    for (int p = sl; p < ncomm; p += SG) { // max gain, ties to the lowest first eligible position = the first-seen rule (:212)
        const int h = spos[p];
        const int c = tk[h], pos = tp[h];
        if (c == old || pos == 0x7fffffff || (pickless && c > old))
            continue;
        const double sacc = ssum[p];
        const double st_c = sum_tot[c];
        lei_best_offer(b, lei_gain(sacc, k_v_to_old, m, resolution, k_v, st_old, st_c), pos, c, sacc - k_v_to_old);
    }
    return lei_best_reduce<SG>(b, old, dk_out);
}

// ── the kernels' argument block, and what they do with a decision ──

struct LeiArgs {
    DevGraph g;
    int *label;
    double *sum_tot;
    const double *kdeg;
    double m, resolution;
    int use_both;
    const int *elig_part; // refinement: phase-1 partition; null for local moving
    int *scratch_c;       // global scratch for nodes with more than LEI_CAP edges: [blocks][max_deg]
    double *scratch_w;
    unsigned char *scratch_e;
    int max_deg;
    int *out; // [0] moves [1] sweeps
    int max_sweeps;
    // batched
    int b0, b1;
    int *dec, *cmin;
    unsigned char *win;
    unsigned char *mv;           // [round slot] 1 = the node wants to move (k_leiden_win scans these instead of dec + label)
    double *dk;
    unsigned long long *Jq, *Lq; // fixed-point (2^20) tallies of the movers' degrees per community
    int apply_on_device;         // 1: unweighted graph, the apply kernels add to sum_tot; 0: weighted, k_leiden_apply_ops has replayed it in node order
    int lds_cap;                 // a wide node (one wavefront): edges staged in LDS (multiple of 16, ≤ LEI_CAP)
    const int *biglist;          // nodes with more than LEI_SG_CAP edges, ascending
    const long long *bigoff;     // [biglist index] offset of the node's region in scratch_c/w/e (nodes with more than LEI_CAP edges)
    int big0, big1;              // the slice of biglist inside [b0, b1)
    int parity;                  // round parity: out[1 + parity] counts this round's safe winners
    int big_log2h;               // table size of a wide node: 2^big_log2h >= lds_cap (one entry per edge at most, so it may fill up)
    int sync;                    // 1: whole-graph synchronous sweep — every positive-gain mover applies, no tallies (k_leiden_apply_sync)
    int pickless;                // this sweep only allows moves to a community with a smaller id
    int sg_log2h;                // log2 of a sub-group's table size (unweighted): LEI_SG_LOG2H, or one less once labels have merged
};

DEVI unsigned long long fx_up(double k) { return (unsigned long long)ceil(k * LEI_FX); }

DEVI int node_degree(const LeiArgs &a, int v) {
    return a.g.off_out[v + 1] - a.g.off_out[v] + (a.use_both ? a.g.off_in[v + 1] - a.g.off_in[v] : 0);
}

// a mover's tallies: smallest mover index per touched community, and the movers' degrees leaving / joining it
DEVI void lei_tally(const LeiArgs &a, int v, int old, int best, double dk) {
    a.dec[v - a.b0] = best;
    if (a.sync) // synchronous sweep: the decision is all k_leiden_apply_sync needs
        return;
    a.dk[v - a.b0] = dk;
    a.mv[v - a.b0] = best != old;
    if (best == old)
        return;
    atomicMin(a.cmin + old, v);
    atomicMin(a.cmin + best, v);
    const unsigned long long q = fx_up(a.kdeg[v]);
    atomicAdd(a.Lq + old, q);
    atomicAdd(a.Jq + best, q);
}
