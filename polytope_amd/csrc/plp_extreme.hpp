// plp_extreme.hpp -- the vertices of a small polytope {A x <= b} (d <= 4, at most 64 rows) by direct enumeration of
// bases: extreme_kernel<D> (plp_extreme.hip) behind plp_extreme_batch.
//
// The contract, as a sequential rule (extreme::one<D> below is that rule; the kernel computes the same list with 64
// candidates at a time):
//   staging     the live rows (i < m, bit i of `keep`) in increasing row index, each scaled to unit 2-norm (a_i / |a_i|,
//               b_i / |a_i|).  A live zero row is not staged: with b_i >= 0 it says nothing, with b_i < 0 (or NaN) the
//               polytope is empty.
//   candidates  every D-subset S = (i0 < i1 < ...) of the n staged rows, in lexicographic order.  S is skipped when
//               |det A_S| <= DET_TOL on the unit rows; else v solves A_S v = b_S (elimination with partial pivoting, the
//               determinant being the product of the pivots).  v is feasible when it is finite and
//               a_i.v - b_i <= FEAS_TOL max(1, |v|_inf, |b_i|) for every staged row.
//   list        the greedy filter of the feasible candidates in that order: a candidate is dropped when a vertex accepted
//               before it lies within SAME_TOL max(1, |v|_inf) of it (max-norm, v the candidate).  Closeness is not
//               transitive, so the rule is sequential on purpose: the list is a function of the input alone.
//   outputs     V[v_max][D] (NaN beyond count), basis[v_max][D] (the ORIGINAL row indices of the accepting subset, -1
//               beyond count), count, status: 0, XS_OVERFLOW (a candidate distinct from the first v_max accepted ones
//               exists: those v_max are written, count = v_max, enumeration stops), XS_EMPTY (no feasible candidate, or
//               an infeasible zero row).
//
// Why these tolerances.  DET_TOL = 1e-12 on unit rows: |det| is the volume of the parallelepiped of the normals, so rows
// that are parallel to 1e-12 rad are one row twice, and v = A_S^-1 b_S of anything better conditioned is known to about
// 1e-16 / |det| <= 1e-4 relative in the worst case, 1e-13 at |det| = 1e-3; a skipped basis loses nothing, because a vertex
// of a bounded polytope is also cut out by some well-conditioned subset of the rows through it, or else the rows through it
// are all parallel to 1e-12 and reduce() has removed all but one of them.  FEAS_TOL = 1e-9 of the extent: the bound the
// library's LP end checks use (plp_support.hpp END_TOL is 1e-10 on one LP; here up to C(64, 4) points are tested and a
// vertex on k > D rows is recomputed from each of its bases, which agree to 1e-16 / |det|).  SAME_TOL = 1e-9 of the
// extent: two bases of one degenerate vertex differ by that rounding, two vertices of a polytope that reduce() has passed
// (rows at least 1e-7 apart in b or direction) by far more.  Rows 1e-7 rad apart that were NOT reduced do cross somewhere
// and give vertices of their own: raw enumeration (reduce=False in Python) returns them.
//
// The same source compiles for the host (g++ -ffp-contract=off, tests/cabi/extreme_host.cpp): sums of products are written
// as separate multiplies and adds in a fixed order, sqrt and / are correctly rounded on both sides, so the device's V is the
// host's bit for bit.
#pragma once
#include "plp_enum.hpp"

namespace plp {
namespace extreme {

constexpr int MAX_DIM = wenum::MAX_DIM, MAX_ROWS = wenum::MAX_ITEMS;
using wenum::binom, wenum::candidates, wenum::next, wenum::unrank;   // (the names they had here before plp_enum.hpp)
constexpr double DET_TOL = 1e-12, FEAS_TOL = 1e-9, SAME_TOL = 1e-9;
enum : int { XS_OK = 0, XS_OVERFLOW = 1, XS_EMPTY = 2 };   // include/plp.h: PLP_XS_*

// LDS (or host scratch) of one polytope: the staged rows [MAX_ROWS][D], their right-hand sides and original indices
constexpr size_t lds_bytes(int D, int m_max) { return (size_t)m_max * (D + 1) * sizeof(double) + (size_t)m_max * sizeof(int); }

// one input row -> its staged form (wenum::unit_row and its verdict; beta = b_i / |a_i|)
template <int D>
PLP_ENUM_FN int stage_row(const double* a, const double bi, double (&u)[D], double& beta) {
    double nrm;
    const int kind = wenum::unit_row<D>(a, bi, u, nrm);
    if (kind == 1) beta = bi / nrm;
    return kind;
}

// A_S v = b_S by elimination with partial pivoting on M = [A_S | b_S], every index a compile-time one.
// -> |det A_S| > DET_TOL (v is only meaningful then)
template <int D>
PLP_ENUM_FN bool solve(double (&M)[D][D + 1], double (&v)[D]) {
    double det = 1.0;
#pragma unroll
    for (int c = 0; c < D; ++c) {
#pragma unroll
        for (int r = c + 1; r < D; ++r) {   // the largest |entry| of column c comes to row c (the first one of equals stays)
            const bool sw = fabs(M[r][c]) > fabs(M[c][c]);
#pragma unroll
            for (int k = 0; k <= D; ++k) {
                const double t = M[c][k];
                M[c][k] = sw ? M[r][k] : t;
                M[r][k] = sw ? t : M[r][k];
            }
        }
        const double piv = M[c][c];
        det = det * piv;
#pragma unroll
        for (int r = c + 1; r < D; ++r) {
            const double f = M[r][c] / piv;
#pragma unroll
            for (int k = c + 1; k <= D; ++k) M[r][k] = M[r][k] - f * M[c][k];
        }
    }
    if (!(fabs(det) > DET_TOL)) return false;
#pragma unroll
    for (int r = D - 1; r >= 0; --r) {
        double s = M[r][D];
#pragma unroll
        for (int k = r + 1; k < D; ++k) s = s - M[r][k] * v[k];
        v[r] = s / M[r][r];
    }
    return true;
}

// the candidate of subset idx on the staged rows sA[n][D], sb[n]: solved, finite and feasible -> v
template <int D>
PLP_ENUM_FN bool candidate(const double* sA, const double* sb, const int n, const int (&idx)[D], double (&v)[D]) {
    double M[D][D + 1];
#pragma unroll
    for (int r = 0; r < D; ++r) {
#pragma unroll
        for (int k = 0; k < D; ++k) M[r][k] = sA[idx[r] * D + k];
        M[r][D] = sb[idx[r]];
    }
    if (!solve<D>(M, v)) return false;
    const double vn = wenum::norm_inf<D>(v);
    if (!(vn < __builtin_inf())) return false;
    const double ext = fmax(1.0, vn);
    bool ok = true;
    for (int i = 0; i < n; ++i) ok = ok & (wenum::dot<D>(sA + i * D, v) - sb[i] <= FEAS_TOL * fmax(ext, fabs(sb[i])));
    return ok;
}

// an accepted vertex w lies within SAME_TOL of the candidate v (the tolerance is the CANDIDATE's)
template <int D>
PLP_ENUM_FN bool same(const double (&v)[D], const double* w) {
    const double tol = SAME_TOL * fmax(1.0, wenum::norm_inf<D>(v));
    bool close = true;
#pragma unroll
    for (int k = 0; k < D; ++k) close = close & (fabs(v[k] - w[k]) <= tol);
    return close;
}

// The whole rule for one polytope, sequentially (the host build; the kernel's answers are held against it bit for bit).
// A[m_max][D], b[m_max], m rows of them in use, keep: bit i = row i is live.  V[v_max][D], basis[v_max][D] or nullptr.
template <int D>
PLP_ENUM_FN void one(const int m_max, const double* A, const double* b, int m, const uint64_t keep, const int v_max, double* V,
                     int* basis, int& count, int& status) {
    double sA[MAX_ROWS * D], sb[MAX_ROWS];
    int sidx[MAX_ROWS];
    m = m < 0 ? 0 : (m > m_max ? m_max : m);
    int n = 0;
    bool empty = false;
    for (int i = 0; i < m; ++i) {
        if (!((keep >> i) & 1)) continue;
        double u[D], beta;
        const int kind = stage_row<D>(A + (size_t)i * D, b[i], u, beta);
        empty = empty | (kind == 2);
        if (kind != 1) continue;
        for (int k = 0; k < D; ++k) sA[n * D + k] = u[k];
        sb[n] = beta;
        sidx[n++] = i;
    }
    count = 0;
    status = XS_OK;
    if (!empty && n >= D) {
        double v[D];   // the candidate the list is looking at
        const bool over = wenum::greedy_list<D>(
            n, v_max, count,
            [&](const int(&idx)[D]) { return candidate<D>(sA, sb, n, idx, v) ? wenum::LIST_TAKE : wenum::LIST_SKIP; },
            [&](const int q) { return same<D>(v, V + (size_t)q * D); },
            [&](const int q, const int(&idx)[D]) {
                for (int k = 0; k < D; ++k) {
                    V[(size_t)q * D + k] = v[k];
                    if (basis) basis[(size_t)q * D + k] = sidx[idx[k]];
                }
            });
        if (over) status = XS_OVERFLOW;
    }
    if (count == 0) status = XS_EMPTY;
    for (size_t q = (size_t)count * D; q < (size_t)v_max * D; ++q) {
        V[q] = __builtin_nan("");
        if (basis) basis[q] = -1;
    }
}

}  // namespace extreme
}  // namespace plp
