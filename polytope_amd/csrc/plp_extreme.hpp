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
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define PLP_XS_FN __host__ __device__ __forceinline__
#else
#define PLP_XS_FN static inline
#endif

namespace plp {
namespace extreme {

constexpr int MAX_DIM = 4, MAX_ROWS = 64;
constexpr double DET_TOL = 1e-12, FEAS_TOL = 1e-9, SAME_TOL = 1e-9;
enum : int { XS_OK = 0, XS_OVERFLOW = 1, XS_EMPTY = 2 };   // include/plp.h: PLP_XS_*

// LDS (or host scratch) of one polytope: the staged rows [MAX_ROWS][D], their right-hand sides and original indices
constexpr size_t lds_bytes(int D, int m_max) { return (size_t)m_max * (D + 1) * sizeof(double) + (size_t)m_max * sizeof(int); }

// C(k, q) for q <= 3 and 0 <= k <= 64 (0 when k < q)
PLP_XS_FN int binom(const int k, const int q) {
    return q == 0 ? 1 : (q == 1 ? k : (q == 2 ? k * (k - 1) / 2 : k * (k - 1) * (k - 2) / 6));
}
// the number of candidates: C(n, D)
template <int D>
PLP_XS_FN int candidates(const int n) {
    return D == 4 ? (int)((long long)binom(n, 3) * (n - 3) / 4) : binom(n, D);
}

// the D-subset of {0 .. n - 1} of lexicographic rank r (0 <= r < C(n, D))
template <int D>
PLP_XS_FN void unrank(const int n, int r, int (&idx)[D]) {
    int c = 0;
#pragma unroll
    for (int pos = 0; pos < D; ++pos) {
        const int q = D - 1 - pos;   // rows still to pick after this one
        if (q == 0) {
            c += r;
        } else {
            for (;;) {
                const int cnt = binom(n - 1 - c, q);
                if (r < cnt) break;
                r -= cnt;
                ++c;
            }
        }
        idx[pos] = c;
        ++c;
    }
}

// the subset after idx in lexicographic order; false when idx was the last
template <int D>
PLP_XS_FN bool next(const int n, int (&idx)[D]) {
    int pos = D - 1;
    while (pos >= 0 && idx[pos] == n - D + pos) --pos;
    if (pos < 0) return false;
    ++idx[pos];
    for (int k = pos + 1; k < D; ++k) idx[k] = idx[k - 1] + 1;
    return true;
}

// one input row -> its staged form.  0: not staged (a zero row that says nothing), 1: staged, 2: the polytope is empty
template <int D>
PLP_XS_FN int stage_row(const double* a, const double bi, double (&u)[D], double& beta) {
    double s = a[0] * a[0];
#pragma unroll
    for (int k = 1; k < D; ++k) s = s + a[k] * a[k];
    const double nrm = sqrt(s);
    if (nrm == 0.0) return bi >= 0.0 ? 0 : 2;
#pragma unroll
    for (int k = 0; k < D; ++k) u[k] = a[k] / nrm;
    beta = bi / nrm;
    return 1;
}

// A_S v = b_S by elimination with partial pivoting on M = [A_S | b_S], every index a compile-time one.
// -> |det A_S| > DET_TOL (v is only meaningful then)
template <int D>
PLP_XS_FN bool solve(double (&M)[D][D + 1], double (&v)[D]) {
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

template <int D>
PLP_XS_FN double norm_inf(const double (&v)[D]) {
    double e = fabs(v[0]);
#pragma unroll
    for (int k = 1; k < D; ++k) e = fmax(e, fabs(v[k]));
    return e;
}

// the candidate of subset idx on the staged rows sA[n][D], sb[n]: solved, finite and feasible -> v
template <int D>
PLP_XS_FN bool candidate(const double* sA, const double* sb, const int n, const int (&idx)[D], double (&v)[D]) {
    double M[D][D + 1];
#pragma unroll
    for (int r = 0; r < D; ++r) {
#pragma unroll
        for (int k = 0; k < D; ++k) M[r][k] = sA[idx[r] * D + k];
        M[r][D] = sb[idx[r]];
    }
    if (!solve<D>(M, v)) return false;
    const double vn = norm_inf<D>(v);
    if (!(vn < __builtin_inf())) return false;
    const double ext = fmax(1.0, vn);
    bool ok = true;
    for (int i = 0; i < n; ++i) {
        double s = sA[i * D] * v[0];
#pragma unroll
        for (int k = 1; k < D; ++k) s = s + sA[i * D + k] * v[k];
        ok = ok & (s - sb[i] <= FEAS_TOL * fmax(ext, fabs(sb[i])));
    }
    return ok;
}

// an accepted vertex w lies within SAME_TOL of the candidate v (the tolerance is the CANDIDATE's)
template <int D>
PLP_XS_FN bool same(const double (&v)[D], const double* w) {
    const double tol = SAME_TOL * fmax(1.0, norm_inf<D>(v));
    bool close = true;
#pragma unroll
    for (int k = 0; k < D; ++k) close = close & (fabs(v[k] - w[k]) <= tol);
    return close;
}

// The whole rule for one polytope, sequentially (the host build; the kernel's answers are held against it bit for bit).
// A[m_max][D], b[m_max], m rows of them in use, keep: bit i = row i is live.  V[v_max][D], basis[v_max][D] or nullptr.
template <int D>
PLP_XS_FN void one(const int m_max, const double* A, const double* b, int m, const uint64_t keep, const int v_max, double* V,
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
        int idx[D];
        for (int k = 0; k < D; ++k) idx[k] = k;
        do {
            double v[D];
            if (!candidate<D>(sA, sb, n, idx, v)) continue;
            bool dup = false;
            for (int q = 0; q < count && !dup; ++q) dup = same<D>(v, V + (size_t)q * D);
            if (dup) continue;
            if (count == v_max) {
                status = XS_OVERFLOW;
                break;
            }
            for (int k = 0; k < D; ++k) {
                V[(size_t)count * D + k] = v[k];
                if (basis) basis[(size_t)count * D + k] = sidx[idx[k]];
            }
            ++count;
        } while (next<D>(n, idx));
    }
    if (count == 0) status = XS_EMPTY;
    for (size_t q = (size_t)count * D; q < (size_t)v_max * D; ++q) {
        V[q] = __builtin_nan("");
        if (basis) basis[q] = -1;
    }
}

}  // namespace extreme
}  // namespace plp
