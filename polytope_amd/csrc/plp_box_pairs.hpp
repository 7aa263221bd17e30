// plp_box_pairs.hpp -- the broad phase of the sparse pair calls (adjacent_pairs_sparse, overlap_pairs_sparse,
// overlap_cross_sparse): which pairs of cells have outer boxes that meet.  The candidate rule, its grid form, and a
// sequential restatement of both for the host.
//
// The rule.  Cell p has the box [lb_p, ub_p] (d values each).  Its padded box is
//     L_p[k] = lb_p[k] - pad * scale_p,   U_p[k] = ub_p[k] + pad * scale_p,   scale_p = max(1, largest finite |bound| of p)
// with loc::cell_range's treatment of the other values (plp_locate.hpp): a NaN bound is -inf / +inf, an infinite bound stays.
// The pair (i, j) is a CANDIDATE iff  max(L_i[k], L_j[k]) <= min(U_i[k], U_j[k])  on all d axes.  That is the definition;
// no grid appears in it.  (A cell whose padded box is empty on some axis -- lb = +inf, ub = -inf -- pairs with nothing.)
//
// Why the cull is exact.  A pair counts iff the stack of the two cells, every right-hand side raised by `inflate`, has a
// Chebyshev radius r > thresh >= 0.  A ball of radius r > 0 then lies in both inflated cells, hence in both of their outer
// boxes, hence in the padded ones: the boxes meet on every axis.  A pair that is no candidate has verdict 0 whatever its LP
// would say.  All this rests on ONE property: every finite box side really bounds {A x <= b + inflate}.
//
// The grid form produces the same set, integer for integer.  With the cell lists of plp_locate.hpp (cell p is listed in
// every grid cell of loc::cell_range(p), built from the SAME boxes and pad), cell i walks the grid cells of its range, meets
// the listed partners j in each and reports (i, j) only from the canonical cell
//     c*_a = max(c_lo_i[a], c_lo_j[a])   on every gridded axis a
// and only if the padded boxes meet on all d axes.  loc::cell_of is monotone, so when the boxes meet on a gridded axis,
// max(L_i, L_j) <= min(U_i, U_j) gives c_lo_i, c_lo_j <= c* <= c_hi_i, c_hi_j: c* lies in both ranges, cell j is listed
// there and cell i walks it.  Every candidate is met there once and reported from nowhere else.
//
// Partners: all pairs -- the j < i; cross form (n1 > 0: the table holds n1 cells and then n - n1) -- cell a < n1 with the
// c >= n1, and cells i >= n1 have no partners.
//
// The same source compiles for the device (plp_box_pairs.hip) and for the host (tests/cabi/box_pairs_host.cpp); both builds
// use -ffp-contract=off.
#pragma once
#include "plp_locate.hpp"

namespace plp {
namespace bp {

using loc::Grid;

// scale_p of the rule: loc::cell_range's
PLP_LOC_FN double box_scale(int d, const double* lb, const double* ub) {
    double scale = 1.0;
    for (int k = 0; k < d; ++k) {
        if (isfinite(lb[k])) scale = fmax(scale, fabs(lb[k]));
        if (isfinite(ub[k])) scale = fmax(scale, fabs(ub[k]));
    }
    return scale;
}

// L_p[k], U_p[k] of the rule from the raw bounds (the arithmetic of loc::cell_range)
PLP_LOC_FN double padded_lo(double l, double pad_scale) {
    if (isnan(l)) l = -INFINITY;
    if (isfinite(l)) l = l - pad_scale;
    return l;
}
PLP_LOC_FN double padded_hi(double u, double pad_scale) {
    if (isnan(u)) u = INFINITY;
    if (isfinite(u)) u = u + pad_scale;
    return u;
}

// the candidate rule; ps_i = pad * scale_i, ps_j = pad * scale_j
PLP_LOC_FN bool boxes_meet(int d, const double* lbi, const double* ubi, double ps_i, const double* lbj, const double* ubj,
                           double ps_j) {
    bool meet = true;
    for (int k = 0; k < d; ++k) {
        const double lo = fmax(padded_lo(lbi[k], ps_i), padded_lo(lbj[k], ps_j));
        const double hi = fmin(padded_hi(ubi[k], ps_i), padded_hi(ubj[k], ps_j));
        meet = meet & (lo <= hi);
    }
    return meet;
}

// the partners cell i is paired with lie in [j_lo, j_hi)
PLP_LOC_FN void partner_range(int n, int n1, int i, int* j_lo, int* j_hi) {
    if (n1 > 0) {
        *j_lo = n1;
        *j_hi = i < n1 ? n : n1;
    } else {
        *j_lo = 0;
        *j_hi = i;
    }
}

// cell j, met in grid cell (c0, c1, c2) on the walk of cell i: is (i, j) reported from here?  (partner, canonical cell,
// padded boxes meet)
PLP_LOC_FN bool walk_hit(const Grid& g, int d, const double* lb, const double* ub, double pad, int i, const int* c_lo_i,
                         double ps_i, int j, int j_lo, int j_hi, int c0, int c1, int c2) {
    if (j < j_lo || j >= j_hi) return false;
    const double* lbj = lb + (size_t)j * d;
    const double* ubj = ub + (size_t)j * d;
    int lo[loc::MAX_AXES], hi[loc::MAX_AXES];
    if (!loc::cell_range(g, d, lbj, ubj, pad, lo, hi)) return false;
    const int s0 = lo[0] > c_lo_i[0] ? lo[0] : c_lo_i[0];
    const int s1 = lo[1] > c_lo_i[1] ? lo[1] : c_lo_i[1];
    const int s2 = lo[2] > c_lo_i[2] ? lo[2] : c_lo_i[2];
    if (s0 != c0 || s1 != c1 || s2 != c2) return false;
    return boxes_meet(d, lb + (size_t)i * d, ub + (size_t)i * d, ps_i, lbj, ubj, pad * box_scale(d, lbj, ubj));
}

#if !defined(__HIPCC__)
// ---- sequential restatement (host only)

// the definition: every partner box-tested.  per_cell[n + 1]: exclusive prefix sums of the partner counts; pairs (NULL:
// count only): (i, j) with cell i's partners ascending
inline void host_brute(int n, int d, const double* lb, const double* ub, double pad, int n1, int64_t* per_cell, int32_t* pairs) {
    int64_t K = 0;
    for (int i = 0; i < n; ++i) {
        per_cell[i] = K;
        int j_lo, j_hi;
        partner_range(n, n1, i, &j_lo, &j_hi);
        const double ps_i = pad * box_scale(d, lb + (size_t)i * d, ub + (size_t)i * d);
        for (int j = j_lo; j < j_hi; ++j) {
            const double ps_j = pad * box_scale(d, lb + (size_t)j * d, ub + (size_t)j * d);
            if (!boxes_meet(d, lb + (size_t)i * d, ub + (size_t)i * d, ps_i, lb + (size_t)j * d, ub + (size_t)j * d, ps_j)) continue;
            if (pairs) { pairs[2 * K] = i; pairs[2 * K + 1] = j; }
            ++K;
        }
    }
    per_cell[n] = K;
}

// the grid walk over the lists cell_start / cell_items (loc::host_grid_count / _fill of the same boxes, pad and grid); a
// cell's partners come out in walk order and are sorted afterwards
inline void host_walk(int n, int d, const double* lb, const double* ub, double pad, const Grid& g, const int32_t* cell_start,
                      const int32_t* cell_items, int n1, int64_t* per_cell, int32_t* pairs) {
    int64_t K = 0;
    for (int i = 0; i < n; ++i) {
        per_cell[i] = K;
        int j_lo, j_hi;
        partner_range(n, n1, i, &j_lo, &j_hi);
        int lo[loc::MAX_AXES], hi[loc::MAX_AXES];
        if (j_lo >= j_hi || !loc::cell_range(g, d, lb + (size_t)i * d, ub + (size_t)i * d, pad, lo, hi)) continue;
        const double ps_i = pad * box_scale(d, lb + (size_t)i * d, ub + (size_t)i * d);
        const int r1 = g.naxes > 1 ? g.res[1] : 1, r2 = g.naxes > 2 ? g.res[2] : 1;
        const int64_t K0 = K;
        for (int c0 = lo[0]; c0 <= hi[0]; ++c0)
            for (int c1 = lo[1]; c1 <= hi[1]; ++c1)
                for (int c2 = lo[2]; c2 <= hi[2]; ++c2) {
                    int c = c0;
                    if (g.naxes > 1) c = c * r1 + c1;
                    if (g.naxes > 2) c = c * r2 + c2;
                    for (int32_t t = cell_start[c]; t < cell_start[c + 1]; ++t) {
                        const int j = cell_items[t];
                        if (j < 0 || j >= n || !walk_hit(g, d, lb, ub, pad, i, lo, ps_i, j, j_lo, j_hi, c0, c1, c2)) continue;
                        if (pairs) { pairs[2 * K] = i; pairs[2 * K + 1] = j; }
                        ++K;
                    }
                }
        if (pairs)  // partners ascending (insertion sort: lists are short)
            for (int64_t t = K0 + 1; t < K; ++t) {
                const int32_t v = pairs[2 * t + 1];
                int64_t u = t - 1;
                while (u >= K0 && pairs[2 * u + 1] > v) { pairs[2 * u + 3] = pairs[2 * u + 1]; --u; }
                pairs[2 * u + 3] = v;
            }
    }
    per_cell[n] = K;
}
#endif

}  // namespace bp
}  // namespace plp
