// plp_reduce_general.hpp -- the general fused reduce, reduce_kernel<D>: one dictionary row per lane, Bland's rule inside
// the simplex (plp_simplex.hpp).  It serves what no fast kernel takes and the second pass that redoes what they hand back
// (RF_RETRY); its tile, reduce_general_tile, is a device function so that the fast kernels can also redo such polytopes
// in place instead of leaving them to a second launch.
//
// Reference behaviour restated (polytope/polytope.py:1053-1163, `reduce`), per polytope; the thresholds and comparisons
// of every step are plp_reduce_rules.hpp's (namespace rule), stated there once for this and the fast kernels:
//   1. is_fulldim -> cheby_ball: LP F1        (:1081, :962-985, :1241-1300)   ball_ok, full_dim, f1_open, empty_flags
//   2. pairwise parallel-row dedupe           (:1094-1112)                    same_plane, row_goes / pair_loser
//   3. early return                           (:1114-1116)                    few_rows
//   4. bounding box = 2 nx LPs F3, prefilter  (:1118-1134, :1367-1409)        box_first, box_optimum / _value, prefilter_add / _drops
//   5. early return                           (:1136-1138)                    few_rows
//   6. one redundancy LP F2 per remaining row (:1142-1160)                    f2_rhs, f2_objective, f2_keeps
// (written out here, each under a comment naming its function: empty_flags, step 3, step 4's read-out and prefilter.  The
// rule for this file: a call may replace them when the lane kernels, whose redo path this tile is, keep their scratch figure.)
// Output: 64-bit keep mask over the INPUT rows, flags, Chebyshev ball, number of LPs solved.
//
// Mapping: a 256-thread workgroup takes a tile of NG = 256/GS polytopes (GS lanes per group,
// GS >= rows).  The tile's rows are read from HBM once, coalesced, into LDS.  Group p then runs
// the whole pipeline of polytope p: lane i keeps row i (a_i, b_i) in VGPRs for the entire
// sequence F1 -> dedupe -> 2d F3 -> prefilter -> one F2 per surviving row; the 64/GS groups of a
// wavefront advance in lockstep, LP by LP.  The LPs of one polytope share everything but the
// objective and one right-hand side entry, so setting one up is a handful of register moves:
//   * F2/F3 start from the dictionary translated to the Chebyshev centre (b - A xc > 0), which is
//     primal feasible: no phase 1;
//   * the optimal value is read off the dictionary (zeta = -negz), not recomputed from x.
// LDS is only read after the staging barrier (row k's coefficients = objective of F2(k), other
// rows for the dedupe), so the groups never synchronise with each other.
// HBM traffic = 8 m (d+1) bytes in + 24 + 8 d bytes out per polytope.
//
// reduce_general_tile:
// NT = threads per workgroup; a tile = NT / gs polytopes (gs lanes per polytope, gs >= rows); smem_raw: at least
// (NT / gs) * gs * (D + 1) doubles.  `mine`: my lane group's polytope takes part (others are left untouched).
#pragma once
#include "plp_kernels.hpp"
#include "plp_reduce_rules.hpp"
#include "plp_simplex.hpp"

namespace plp {

template <int D, int NT>
__device__ __forceinline__ void reduce_general_tile(unsigned char* smem_raw, const long long tile, const int ntile, const bool mine,
                                                    int m_max, int gs, const double* __restrict__ Ag,
                                                    const double* __restrict__ bg, const int* __restrict__ mrows,
                                                    double abs_tol, unsigned long long* __restrict__ keep_out,
                                                    int* __restrict__ flags_out, double* __restrict__ r_out,
                                                    double* __restrict__ xc_out, int* __restrict__ nlp_out) {
    const Grp g(gs);
    const int NG = NT / gs;
    const int gib = threadIdx.x / gs;
    const int i = g.gl;
    double* sA = reinterpret_cast<double*>(smem_raw);   // [NG][gs][D]
    double* sb = sA + (size_t)NG * gs * D;               // [NG][gs]
    const double* myA = sA + (size_t)gib * gs * D;       // rows of my polytope
    const double* myb = sb + (size_t)gib * gs;
    using rule::qnan;
    using rule::pinf;
    // ---------------------------------------------------------------- stage rows in LDS
    __syncthreads();  // the previous tile's readers are done
    {
        const int rowsz = m_max * D;
        const int totA = ntile * rowsz;
        const double* src = Ag + tile * rowsz;
        for (int idx = threadIdx.x; idx < totA; idx += NT) {
            const int p = idx / rowsz, rem = idx - p * rowsz;
            const int row = rem / D, k = rem - row * D;
            sA[((size_t)p * gs + row) * D + k] = src[idx];
        }
        const int totb = ntile * m_max;
        const double* srcb = bg + tile * m_max;
        for (int idx = threadIdx.x; idx < totb; idx += NT) {
            const int p = idx / m_max, row = idx - p * m_max;
            sb[p * gs + row] = srcb[idx];
        }
    }
    __syncthreads();
    const long long pg = tile + gib;
    const bool valid = gib < ntile && mine;
    const int m = valid ? (mrows ? mrows[pg] : m_max) : 0;
    const bool has_row = valid && i < m && m <= gs;
    // ---------------------------------------------------------------- my row
    double a[D];
#pragma unroll
    for (int k = 0; k < D; ++k) a[k] = has_row ? myA[i * D + k] : 0.0;
    const double bi = has_row ? myb[i] : 0.0;
    // ---------------------------------------------------------------- F1: Chebyshev ball (cheby_lp, plp_simplex.hpp)
    double xc[D];
    double rr = 0.0, an_i;
    bool ball, fulldim, f1open = false;
    {
        double x1[D + 1];
        const int st1 = cheby_lp<D>(g, valid, has_row, m, gs, a, bi, x1, an_i);
        f1open = valid && rule::f1_open(st1);
#pragma unroll
        for (int j = 0; j < D; ++j) xc[j] = x1[j];
        rr = x1[D];
        ball = rule::ball_ok(st1, rr);
        {   // a centre that violates a row (centre_off, plp_common.hpp) is no centre: RF_F1OPEN
            double sk = 0.0;
#pragma unroll
            for (int k = 0; k < D; ++k) sk = fma(a[k], xc[k], sk);
            if (ball && grp_ballot(has_row && centre_off(bi - sk, an_i, bi, centre_scale<D>(xc)), g) != 0) {
                ball = false; f1open = true;
            }
        }
        fulldim = rule::full_dim(ball, rr, abs_tol);
    }
    // ---------------------------------------------------------------- dedupe (:1094-1110)
    uint64_t live;
    {
        bool removed = false;
        double ni[D];
#pragma unroll
        for (int k = 0; k < D; ++k) ni[k] = a[k] * an_i;
        const double bin_ = bi * an_i;
        for (int j = 0; j < m_max; ++j) {
            const bool jrow = valid && j < m;
            const double an_j = bcast(an_i, g.gbase + (j & (gs - 1)));
            double dot = 0.0;
#pragma unroll
            for (int k = 0; k < D; ++k) dot = dot + ni[k] * (myA[j * D + k] * an_j);
            const double bjn = myb[j] * an_j;
            const bool par = has_row && jrow && j != i && rule::same_plane(dot, abs_tol);
            removed = removed || (par && rule::row_goes(i, j, bin_, bjn));
        }
        live = grp_ballot(has_row && !removed, g);
    }
    int flags = fulldim ? 0 : (RF_EMPTY | (f1open ? RF_F1OPEN : 0));   // rule::empty_flags WRITTEN OUT (see the top)
    int nlp = 1;
    uint64_t keep = 0ull;
    int stage = 0;  // 0 done, 1 needs the box, 2 needs the redundancy LPs
    if (fulldim) {
        const int neq = __popcll(live);   // rule::few_rows / rule::box_first WRITTEN OUT
        if (neq <= D + 1) { flags = RF_EARLY; keep = live; }
        else stage = (neq > 3 * D) ? 1 : 2;
    }
    // dictionary translated to the Chebyshev centre: beta_i = b_i - a_i.xc
    double s = 0.0;
#pragma unroll
    for (int k = 0; k < D; ++k) s = fma(a[k], ball ? xc[k] : 0.0, s);
    // ---------------------------------------------------------------- F3: bounding box (:1367-1409)
    if (__any(stage == 1)) {
        double s1 = 0.0, s2 = 0.0;
        bool lpfail = false;
        const bool lrow = (live >> i) & 1ull;
        const double bsh = bi - s;
        const bool go = stage == 1;
        double lbk = 0.0;
        for (int it = 0; it < 2 * D; ++it) {  // lower_0, upper_0, lower_1, upper_1, ...
            const int k = it >> 1;
            const bool up = it & 1;
            double aik = 0.0, xck = 0.0;
            Simplex<D, false, false> S;
            S.reset(D, __popcll(live), i);
#pragma unroll
            for (int kk = 0; kk < D; ++kk) {
                aik = (kk == k) ? a[kk] : aik;
                xck = (kk == k) ? xc[kk] : xck;
                S.T[kk] = lrow ? a[kk] : 0.0;
                S.cost[kk] = (kk == k) ? (up ? -1.0 : 1.0) : 0.0;
            }
            S.beta = (lrow && bsh > 0.0) ? bsh : 0.0;
            S.rowact = lrow;
            S.mode = go ? M_P2 : M_DONE;
            S.run(g);
            // rule::box_optimum / box_value, prefilter_add / prefilter_drops WRITTEN OUT (the lane kernels' redo path, as above)
            double val;
            if (S.status == ST_OPT) val = up ? (xck + S.negz) : (xck - S.negz);
            else if (S.status == ST_UNBND) val = up ? pinf : -pinf;
            else { val = qnan; lpfail = lpfail || go; }
            if (!up) {
                lbk = val;
            } else {  // prefilter sums, accumulated in k order (:1131-1134)
                const double pa = (aik > 0.0 ? 1.0 : 0.0) * aik;
                s1 = s1 + pa * (val - lbk);
                s2 = s2 + aik * lbk;
            }
        }
        const bool out = (s1 - (bi - s2)) < -1e-4;
        const uint64_t outb = grp_ballot(go && lrow && out, g);
        if (go) {
            live = live & ~outb;
            nlp += 2 * D;
            if (lpfail) flags |= RF_LPFAIL;
            if (rule::few_rows(__popcll(live), D)) { flags |= RF_EARLY; keep = live; stage = 0; }
            else stage = 2;
        }
    }
    // ---------------------------------------------------------------- F2: redundancy LPs (:1142-1160)
    if (__any(stage == 2)) {
        const bool lrow = (live >> i) & 1ull;
        uint64_t todo = (stage == 2) ? live : 0ull;
        if (stage == 2) nlp += __popcll(live);
        while (__any(todo != 0ull)) {
            const bool go = todo != 0ull;
            const int k = go ? __ffsll((long long)todo) - 1 : 0;
            todo &= todo - 1ull;
            Simplex<D, false, false> S;
            S.reset(D, __popcll(live), i);
            double cxc = 0.0;
#pragma unroll
            for (int kk = 0; kk < D; ++kk) {
                const double ck = -myA[k * D + kk];  // f = -A[k,:]  (:1145)
                S.T[kk] = lrow ? a[kk] : 0.0;
                S.cost[kk] = ck;
                cxc = fma(ck, xc[kk], cxc);
            }
            const double bsh = rule::f2_rhs(i < k, i == k, bi) - s;   // rows before k carry the round trip
            S.beta = (lrow && bsh > 0.0) ? bsh : 0.0;
            S.rowact = lrow;
            S.mode = go ? M_P2 : M_DONE;
            S.run(g);
            const double fun = cxc - S.negz;        // c.xc + zeta, zeta = -negz
            const double obj = rule::f2_objective(fun, rule::rhs_round_trip(myb[k]));
            const bool keepk = go && rule::f2_keeps(S.status, obj, abs_tol);
            keep |= keepk ? (1ull << k) : 0ull;
        }
        if (stage == 2) flags |= RF_MINREP;
    }
    // ---------------------------------------------------------------- results
    if (valid && i == 0) {
        keep_out[pg] = keep;
        flags_out[pg] = flags;
        nlp_out[pg] = nlp;
        r_out[pg] = ball ? rr : 0.0;
    }
    if (valid) {
#pragma unroll
        for (int k = 0; k < D; ++k)
            if (i == (k & (gs - 1)) ) xc_out[pg * D + k] = ball ? xc[k] : qnan;
    }
}

// Waves per SIMD the register allocator must leave room for (2nd __launch_bounds__ argument).
// Measured on MI355X at d=3 (100k polytopes, m=16): 3 waves 0.820 ms, 4 waves 0.719 ms,
// 5 waves 0.703 ms (24 VGPRs spilled outside the pivot loop), 6 waves 0.706 ms: the kernel is
// VALU-issue bound from ~4 waves on, and the 5/6-wave builds pay for their spills with scratch
// traffic (WRITE_SIZE 4.7 MB -> 132 MB per launch).  Larger d needs the registers more than the
// occupancy.
#ifndef PLP_REDUCE_WAVES
#define PLP_REDUCE_WAVES(D) ((D) <= 4 ? 4 : ((D) <= 8 ? 3 : 2))
#endif

template <int D>
__global__ __launch_bounds__(BLOCK, PLP_REDUCE_WAVES(D)) void reduce_kernel(long long B, int m_max, int gs,
                                                       const double* __restrict__ Ag,
                                                       const double* __restrict__ bg,
                                                       const int* __restrict__ mrows, double abs_tol,
                                                       int retry_only,
                                                       unsigned long long* __restrict__ keep_out,
                                                       int* __restrict__ flags_out,
                                                       double* __restrict__ r_out,
                                                       double* __restrict__ xc_out,
                                                       int* __restrict__ nlp_out,
                                                       const unsigned long long* __restrict__ retry_word,
                                                       unsigned long long epoch) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    // second pass: the fast kernels raise the call's word when they hand a polytope back; normally they did not
    // The word lives in a ring of 64 (slot = epoch & 63, raised with atomicMax): a value BELOW this call's epoch means no
    // tile of this call asked for the second pass; this call's own epoch means some did; a LARGER value is a later call
    // (64 or more calls of one context in flight on other streams) that took the slot over -- then nothing is known and
    // the flags of the batch are swept as if the word were not there.
    if (retry_only && retry_word && *retry_word < epoch) return;
    const int NG = BLOCK / gs;
    const int gib = threadIdx.x / gs;

    if (retry_only) {
        // normally nothing was handed back: all flag loads of this workgroup's tiles are issued at once (one
        // memory round trip instead of one per tile of the sweep below) and the workgroup leaves
        bool any = false;
        for (long long tile = (long long)blockIdx.x * NG; tile < B; tile += (long long)gridDim.x * NG)
            any = any | ((tile + gib < B) && (flags_out[tile + gib] & RF_RETRY) != 0);
        if (!__syncthreads_or(any)) return;
    }
    for (long long tile = (long long)blockIdx.x * NG; tile < B; tile += (long long)gridDim.x * NG) {
        const int ntile = (B - tile) < NG ? (int)(B - tile) : NG;
        // second pass after reduce_r_kernel: only polytopes it flagged RF_RETRY (tiles without one are skipped)
        bool mine = true;
        if (retry_only) {
            mine = (gib < ntile) && (flags_out[tile + gib] & RF_RETRY) != 0;
            if (!__syncthreads_or(mine)) continue;
        }
        reduce_general_tile<D, BLOCK>(smem_raw, tile, ntile, mine, m_max, gs, Ag, bg, mrows, abs_tol, keep_out, flags_out, r_out,
                                      xc_out, nlp_out);
    }
}

}  // namespace plp
