// plp_locate.hpp -- the arithmetic of point location (locate_batch: first containing polytope per point, and how many
// contain it): the row test in contains_kernel's arithmetic (plp_points.hip), the uniform grid that culls the candidates,
// and a sequential restatement of the grid's count / fill / query passes.
//
// The dense answer is the definition: first[q] = min { p : all_i<m[p] (fl(A_p[i].x_q) - b_p[i]) < tol }, or -1, and
// count[q] the number of such p; the dot product is s = a0 x0, s = fma(a_k, x_k, s) with k ascending.  A polytope without
// rows contains every point (NaN points too); a NaN coordinate fails every row it meets.
//
// The grid.  Up to MAX_AXES coordinate axes are cut into res_j equal cells from lo_j on; a point's cell along axis j is
//     cell_j(x) = (int) fmin(fmax(floor((x - lo_j) * inv_h_j), 0), res_j - 1)            (NaN -> 0)
// and a polytope is listed in every cell of  [cell_j(lb_j - pad), cell_j(ub_j + pad)]  over the gridded axes, [lb, ub] its
// bounding box and pad a relative allowance (pad * max(1, the box's largest finite |bound| on any axis)).
// cell_j is MONOTONE NON-DECREASING in x -- x - lo,
// the product with inv_h >= 0, floor and the two clamps all are, also at +-inf (inv_h = 0 makes every finite x cell 0, and
// inf * 0 = NaN is cell 0 as well) -- so lb - pad <= x <= ub + pad implies cell(lb - pad) <= cell(x) <= cell(ub + pad):
// the cull never loses a polytope whose padded box holds the point.  That is all its correctness rests on; which axes,
// which resolution and which pad only decide how long the lists are.  Points outside the grid's domain land in the border
// cells, where every polytope reaching beyond the domain is listed too (its range is clamped the same way).
// A NaN point sits in cell 0 of that axis and fails every row: it is inside rowless polytopes only, and those are listed
// everywhere (infinite box).
//
// The same source compiles for the device (plp_locate.hip) and for the host (tests/cabi/locate_host.cpp); both builds use
// -ffp-contract=off, so the only fused operations are the fma() calls.
#pragma once
#include <math.h>
#include <stdint.h>

#include "../../include/plp.h"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define PLP_LOC_FN __host__ __device__ __forceinline__
#else
#define PLP_LOC_FN inline
#endif

namespace plp {
namespace loc {

constexpr int MAX_AXES = PLP_LOCATE_MAX_AXES;
constexpr int MAX_CELLS = PLP_LOCATE_MAX_CELLS;

typedef plp_locate_grid Grid;

// one row against one point: contains_kernel's arithmetic
template <int D>
PLP_LOC_FN bool row_inside(const double* a, double bi, const double* x, double tol) {
    double s = a[0] * x[0];
#pragma unroll
    for (int k = 1; k < D; ++k) s = fma(a[k], x[k], s);
    return (s - bi) < tol;
}

// the same with the dimension at run time (host restatement)
PLP_LOC_FN bool row_inside_n(int d, const double* a, double bi, const double* x, double tol) {
    double s = a[0] * x[0];
    for (int k = 1; k < d; ++k) s = fma(a[k], x[k], s);
    return (s - bi) < tol;
}

// the cell of coordinate x along one gridded axis; monotone non-decreasing in x, NaN -> 0
PLP_LOC_FN int cell_of(double x, double lo, double inv_h, int res) {
    return (int)fmin(fmax(floor((x - lo) * inv_h), 0.0), (double)(res - 1));
}

PLP_LOC_FN int n_cells(const Grid& g) {
    int G = 1;
    for (int j = 0; j < g.naxes; ++j) G *= g.res[j];
    return G;
}

// 0 when the descriptor is usable for points of dimension d
PLP_LOC_FN int grid_bad(const Grid& g, int d) {
    if (g.naxes < 1 || g.naxes > MAX_AXES) return 1;
    long long G = 1;
    for (int j = 0; j < g.naxes; ++j) {
        if (g.axis[j] < 0 || g.axis[j] >= d || g.res[j] < 1 || !(g.inv_h[j] >= 0.0) || isnan(g.lo[j])) return 1;
        for (int i = 0; i < j; ++i)
            if (g.axis[i] == g.axis[j]) return 1;
        G *= g.res[j];
        if (G > MAX_CELLS) return 1;
    }
    return 0;
}

// the flat cell of a point (x[k]: coordinate k; `stride` elements apart, so a column of X[d][N] is read in place)
PLP_LOC_FN int point_cell(const Grid& g, const double* x, long long stride) {
    int c = 0;
    for (int j = 0; j < g.naxes; ++j) c = c * g.res[j] + cell_of(x[(long long)g.axis[j] * stride], g.lo[j], g.inv_h[j], g.res[j]);
    return c;
}

// the cell range of a polytope with box [lb, ub] (d values each).  false: listed nowhere -- the padded box is empty on a
// gridded axis (lb - pad' > ub + pad'; a caller marks "contains nothing" as lb = +inf, ub = -inf).  Infinite sides, and
// lb = -inf / ub = +inf for "box unknown", give the whole axis.  NaN bounds: the whole axis as well (cell(NaN) = 0 would
// be wrong for an upper bound, so they are replaced by the infinities first).
// pad' = pad * max(1, the largest finite |bound| of the box on ANY axis): the rounding of fl(a . x) of a tilted row goes
// with the largest coordinate of the point, not with the one along the gridded axis.
PLP_LOC_FN bool cell_range(const Grid& g, int d, const double* lb, const double* ub, double pad, int* c_lo, int* c_hi) {
    double scale = 1.0;
    for (int k = 0; k < d; ++k) {
        if (isfinite(lb[k])) scale = fmax(scale, fabs(lb[k]));
        if (isfinite(ub[k])) scale = fmax(scale, fabs(ub[k]));
    }
    for (int j = 0; j < g.naxes; ++j) {
        double l = lb[g.axis[j]], u = ub[g.axis[j]];
        if (isnan(l)) l = -INFINITY;
        if (isnan(u)) u = INFINITY;
        if (isfinite(l)) l = l - pad * scale;
        if (isfinite(u)) u = u + pad * scale;
        if (l > u) return false;
        c_lo[j] = cell_of(l, g.lo[j], g.inv_h[j], g.res[j]);
        c_hi[j] = cell_of(u, g.lo[j], g.inv_h[j], g.res[j]);
    }
    for (int j = g.naxes; j < MAX_AXES; ++j) c_lo[j] = c_hi[j] = 0;
    return true;
}

// f(flat cell) for every cell of the range, row-major over the gridded axes as point_cell numbers them
template <typename F>
PLP_LOC_FN void for_cells(const Grid& g, const int* c_lo, const int* c_hi, F f) {
    const int r1 = g.naxes > 1 ? g.res[1] : 1, r2 = g.naxes > 2 ? g.res[2] : 1;
    for (int i0 = c_lo[0]; i0 <= c_hi[0]; ++i0)
        for (int i1 = c_lo[1]; i1 <= c_hi[1]; ++i1)
            for (int i2 = c_lo[2]; i2 <= c_hi[2]; ++i2) {
                int c = i0;
                if (g.naxes > 1) c = c * r1 + i1;
                if (g.naxes > 2) c = c * r2 + i2;
                f(c);
            }
}

#if !defined(__HIPCC__)
// ---- sequential restatement (host only): what the kernels of plp_locate.hip compute, the plain way

// cell_start[G + 1]: exclusive prefix sums of the list lengths (saturating at INT32_MAX); *max_len: the longest list
inline void host_grid_count(const Grid& g, int P, int d, const double* lb, const double* ub, double pad, int32_t* cell_start,
                            int32_t* max_len) {
    const int G = n_cells(g);
    for (int c = 0; c <= G; ++c) cell_start[c] = 0;
    for (int p = 0; p < P; ++p) {
        int lo[MAX_AXES], hi[MAX_AXES];
        if (!cell_range(g, d, lb + (size_t)p * d, ub + (size_t)p * d, pad, lo, hi)) continue;
        for_cells(g, lo, hi, [&](int c) { cell_start[c + 1] += 1; });
    }
    long long run = 0;
    int32_t mx = 0;
    for (int c = 0; c < G; ++c) {
        const int32_t n = cell_start[c + 1];
        mx = n > mx ? n : mx;
        run += n;
        cell_start[c + 1] = run > 2147483647ll ? 2147483647 : (int32_t)run;
    }
    *max_len = mx;
}

// cell_items[cell_start[G]]: the polytopes of every cell, ascending (polytopes are visited in ascending order)
inline void host_grid_fill(const Grid& g, int P, int d, const double* lb, const double* ub, double pad, const int32_t* cell_start,
                           int32_t* cursor, int32_t* cell_items) {
    const int G = n_cells(g);
    for (int c = 0; c < G; ++c) cursor[c] = 0;
    for (int p = 0; p < P; ++p) {
        int lo[MAX_AXES], hi[MAX_AXES];
        if (!cell_range(g, d, lb + (size_t)p * d, ub + (size_t)p * d, pad, lo, hi)) continue;
        for_cells(g, lo, hi, [&](int c) { cell_items[cell_start[c] + cursor[c]++] = p; });
    }
}

inline bool host_inside(int m_max, int d, const double* A, const double* b, const int32_t* m, int p, const double* x, double tol) {
    const int mp = m ? m[p] : m_max;
    for (int i = 0; i < mp; ++i)
        if (!row_inside_n(d, A + ((size_t)p * m_max + i) * d, b[(size_t)p * m_max + i], x, tol)) return false;
    return true;
}

// first[N] (and count[N] unless NULL) of the points X[d][N]; g == NULL: every polytope is a candidate
inline void host_locate(int P, int m_max, int d, const double* A, const double* b, const int32_t* m, long long N, const double* X,
                        double tol, const Grid* g, const int32_t* cell_start, const int32_t* cell_items, int32_t* first,
                        int32_t* count) {
    for (long long q = 0; q < N; ++q) {
        double x[16];
        for (int k = 0; k < d; ++k) x[k] = X[(long long)k * N + q];
        int32_t f = -1, n = 0;
        if (g) {
            const int c = point_cell(*g, x, 1);
            for (int32_t t = cell_start[c]; t < cell_start[c + 1]; ++t) {
                const int p = cell_items[t];
                if (host_inside(m_max, d, A, b, m, p, x, tol)) { f = f < 0 ? p : f; ++n; }
            }
        } else {
            for (int p = 0; p < P; ++p)
                if (host_inside(m_max, d, A, b, m, p, x, tol)) { f = f < 0 ? p : f; ++n; }
        }
        first[q] = f;
        if (count) count[q] = n;
    }
}
#endif

}  // namespace loc
}  // namespace plp
