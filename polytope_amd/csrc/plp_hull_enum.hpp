// plp_hull_enum.hpp -- the facets of a small point set (d <= 4, at most 64 points) by direct enumeration of hyperplanes:
// hull_enum_kernel<D> (plp_hull_enum.hip) behind plp_hull_batch.  (plp_hull.hip is quickhull's reassignment kernel: another
// thing.)
//
// The contract, as a sequential rule (hullenum::one<D> below is that rule; the kernel computes the same list with 64
// candidates at a time):
//   staging     the live points (i < n, bit i of `keep`) in increasing index.  c = (min + max) / 2 per coordinate over them,
//               s = the largest |p_i - c|_inf: min and max do not depend on the order they are taken in, so a wave
//               reduction and a loop give the same bits (c + 0.0 makes a zero centre +0 whichever zero min / max returned).
//               FLAT when s is not a positive finite number or fewer than D + 1 points are live.  Else q_i = (p_i - c) / s:
//               every coordinate lies in [-1, 1], and the tolerances below are absolute on the q.
//   candidates  every D-subset S = (i0 < i1 < ...) of the staged points, in lexicographic order (unrank / next / binom of
//               plp_enum.hpp).  Edges e_k = q_ik - q_i0, k = 1 .. D - 1; the normal nu is their generalised cross
//               product (normal<D> below fixes the order of operations: D = 1: 1, D = 2: (e_y, -e_x), D = 3: e1 x e2,
//               D = 4: the signed 3 x 3 cofactors of [e1; e2; e3]).  S is skipped unless |nu|_2 > DEG_TOL prod |e_k|_2 --
//               which also skips a zero edge (both sides 0) and anything that is not a number.  Else nu <- nu / |nu|_2,
//               off = nu.q_i0, r_i = nu.q_i - off over ALL staged points, and with hi = max r, lo = min r:
//                 hi <= SIDE_TOL and lo >= -SIDE_TOL   every point lies on this plane: the set is flat, enumeration ends;
//                 hi <= SIDE_TOL                        the facet (nu, off);
//                 lo >= -SIDE_TOL                       the facet (-nu, -off);
//                 otherwise                             no facet.
//   list        the greedy filter of the facets in that order: a facet is dropped when one accepted BEFORE it has
//               |nu - nu'|_inf <= SAME_TOL and |off - off'| <= SAME_TOL.  A face that carries more than D points is cut out
//               by every D-subset of them in general position and is reported once.
//   outputs     per accepted facet the row in the CALLER's coordinates: Ao[f_max][D] = nu (unit 2-norm),
//               bo[f_max] = nu.c + s off (the dot product summed in index order), on[f_max]: bit i set when the original
//               point i is live and |r_i| <= SIDE_TOL (the facet's incidence), basis[f_max][D] (optional): the ORIGINAL
//               indices of the accepting subset.  Beyond count: NaN, NaN, 0, -1.
//               status: 0; HS_OVERFLOW (a facet distinct from the first f_max accepted ones exists: those f_max are
//               written, count = f_max, enumeration stops there); HS_FLAT (count = 0: see staging and candidates; also
//               when no candidate survives the skip).
//
// Why these tolerances.  All three are absolute on coordinates scaled to [-1, 1].  DEG_TOL = 1e-12 is the sine of the
// "angle" of the subset: |nu| / prod |e_k| is the volume of the parallelepiped of the unit edges.  Low is the safe side: a
// subset that is skipped wrongly can lose a facet, and a lost facet opens the hull, whereas a subset that is kept wrongly
// cannot add a wrong row -- its plane is computed with a relative error of about 1e-16 / sine (1e-4 at the threshold), but
// every plane, however it was found, is tested against all the points, so a row that comes out is valid to SIDE_TOL by
// construction.  At worst a sliver subset of a face re-finds that face's row a little tilted, more than SAME_TOL from the
// row already accepted: a near-duplicate row, never a wrong one.  A face of the hull with more than D points has a subset
// far better conditioned than 1e-12 unless all its points are collinear to 1e-12, and then it is no (D - 1)-face.
// SIDE_TOL = 1e-9: r_i of a point on the plane of a well-conditioned subset is off by a few 1e-16 (d <= 4 products of
// numbers <= 2, one division), of a subset of sine 1e-6 by 1e-10; 1e-9 accepts those and is two orders below the 1e-7 at
// which the library elsewhere (and the reference's quickhull) calls a point "on" a plane, so what is a facet here is one
// there.  It is also what "flat" means: a set whose thickness is below 1e-9 of its extent.  SAME_TOL = 1e-9: two
// well-conditioned subsets of one face give rows that agree to about 1e-15; two distinct facets of a hull whose points are
// at least SIDE_TOL off each other's planes differ by more.  Closeness is not transitive, so the filter is sequential on
// purpose: the list is a function of the input alone.
//
// The same source compiles for the host (g++ -ffp-contract=off, tests/cabi/hull_enum_host.cpp): sums of products are
// written as separate multiplies and adds in a fixed order, sqrt and / are correctly rounded on both sides, so the device's
// rows are the host's bit for bit.
#pragma once
#include "plp_enum.hpp"

namespace plp {
namespace hullenum {

constexpr int MAX_DIM = wenum::MAX_DIM, MAX_POINTS = wenum::MAX_ITEMS;
constexpr double DEG_TOL = 1e-12, SIDE_TOL = 1e-9, SAME_TOL = 1e-9;
enum : int { HS_OK = 0, HS_OVERFLOW = 1, HS_FLAT = 2 };   // include/plp.h: PLP_HS_*
enum : int { CAND_NONE = 0, CAND_FACET = 1, CAND_FLAT = 2 };

// LDS (or host scratch) of one point set: the staged points [n_max][D] and their original indices
constexpr size_t lds_bytes(int D, int n_max) { return (size_t)n_max * D * sizeof(double) + (size_t)n_max * sizeof(int); }

// the centre of [lo, hi] (a zero is +0) and a point's distance from it in the max-norm
PLP_ENUM_FN double centre(const double lo, const double hi) { return (lo + hi) / 2.0 + 0.0; }
template <int D>
PLP_ENUM_FN double reach(const double (&p)[D], const double (&c)[D]) {
    double e = fabs(p[0] - c[0]);
#pragma unroll
    for (int k = 1; k < D; ++k) e = fmax(e, fabs(p[k] - c[k]));
    return e;
}
// is this (s, live points) a set the enumeration takes?
template <int D>
PLP_ENUM_FN bool stageable(const double s, const int live) {
    return s > 0.0 && s < __builtin_inf() && live >= D + 1;
}

// a1 (b2 c3 - b3 c2) - a2 (b1 c3 - b3 c1) + a3 (b1 c2 - b2 c1): the determinant of the columns a, b, c
PLP_ENUM_FN double det3(const double a1, const double a2, const double a3, const double b1, const double b2, const double b3,
                        const double c1, const double c2, const double c3) {
    const double t1 = a1 * (b2 * c3 - b3 * c2);
    const double t2 = a2 * (b1 * c3 - b3 * c1);
    const double t3 = a3 * (b1 * c2 - b2 * c1);
    return (t1 - t2) + t3;
}

// The generalised cross product of the edges e[1 .. D - 1] (e[0] is not used) -> nu, and prod |e_k|_2.
template <int D>
PLP_ENUM_FN double normal(const double (&e)[D][D], double (&nu)[D]) {
    double prod = 1.0;
#pragma unroll
    for (int k = 1; k < D; ++k) prod = prod * sqrt(wenum::dot<D>(e[k], e[k]));
    if constexpr (D == 1) {
        nu[0] = 1.0;
    } else if constexpr (D == 2) {
        nu[0] = e[1][1];
        nu[1] = -e[1][0];
    } else if constexpr (D == 3) {
        const double(&a)[D] = e[1];
        const double(&b)[D] = e[2];
        nu[0] = a[1] * b[2] - a[2] * b[1];
        nu[1] = a[2] * b[0] - a[0] * b[2];
        nu[2] = a[0] * b[1] - a[1] * b[0];
    } else {
        // column j of the 3 x 4 matrix [e1; e2; e3] is (e[1][j], e[2][j], e[3][j]); nu_k = (-1)^k det(all columns but k)
        const double(&a)[D] = e[1];
        const double(&b)[D] = e[2];
        const double(&c)[D] = e[3];
        nu[0] = det3(a[1], b[1], c[1], a[2], b[2], c[2], a[3], b[3], c[3]);
        nu[1] = -det3(a[0], b[0], c[0], a[2], b[2], c[2], a[3], b[3], c[3]);
        nu[2] = det3(a[0], b[0], c[0], a[1], b[1], c[1], a[3], b[3], c[3]);
        nu[3] = -det3(a[0], b[0], c[0], a[1], b[1], c[1], a[2], b[2], c[2]);
    }
    return prod;
}

// The candidate of subset idx on the staged points sq[n][D] (sidx[n]: their original indices) -> CAND_*; for a facet
// (nu, off) is the row on the staged points, oriented, and `on` its incidence word.
template <int D>
PLP_ENUM_FN int candidate(const double* sq, const int* sidx, const int n, const int (&idx)[D], double (&nu)[D], double& off,
                          uint64_t& on) {
    double e[D][D];
#pragma unroll
    for (int k = 1; k < D; ++k) {
#pragma unroll
        for (int j = 0; j < D; ++j) e[k][j] = sq[idx[k] * D + j] - sq[idx[0] * D + j];
    }
    const double prod = normal<D>(e, nu);
    const double nn = sqrt(wenum::dot<D>(nu, nu));
    if (!(nn > DEG_TOL * prod)) return CAND_NONE;
#pragma unroll
    for (int j = 0; j < D; ++j) nu[j] = nu[j] / nn;
    off = wenum::dot<D>(nu, sq + idx[0] * D);
    double hi = -__builtin_inf(), lo = __builtin_inf();
    uint64_t w = 0;
    for (int i = 0; i < n; ++i) {
        const double r = wenum::dot<D>(nu, sq + i * D) - off;
        hi = fmax(hi, r);
        lo = fmin(lo, r);
        w |= (uint64_t)(fabs(r) <= SIDE_TOL) << sidx[i];
    }
    on = w;
    const bool below = hi <= SIDE_TOL, above = lo >= -SIDE_TOL;
    if (below && above) return CAND_FLAT;
    if (!below && !above) return CAND_NONE;
    if (!below) {
#pragma unroll
        for (int j = 0; j < D; ++j) nu[j] = -nu[j];
        off = -off;
    }
    return CAND_FACET;
}

// an accepted facet (w, woff) is the candidate's row to SAME_TOL
template <int D>
PLP_ENUM_FN bool same(const double (&nu)[D], const double off, const double* w, const double woff) {
    bool close = fabs(off - woff) <= SAME_TOL;
#pragma unroll
    for (int k = 0; k < D; ++k) close = close & (fabs(nu[k] - w[k]) <= SAME_TOL);
    return close;
}

// an accepted row (nu, off) on the staged points -> its right-hand side in the caller's coordinates
template <int D>
PLP_ENUM_FN double unstage(const double* nu, const double off, const double (&c)[D], const double s) {
    return wenum::dot<D>(nu, c) + s * off;
}

// The whole rule for one point set, sequentially (the host build; the kernel's answers are held against it bit for bit).
// X[n_max][D], n points of them in use, keep: bit i = point i is live.  Ao[f_max][D], bo[f_max], on[f_max], basis[f_max][D]
// or nullptr.  While the enumeration runs bo holds `off` of the accepted rows, as it does in the kernel.
template <int D>
PLP_ENUM_FN void one(const int n_max, const double* X, int n, const uint64_t keep, const int f_max, double* Ao, double* bo,
                     uint64_t* on, int* basis, int& count, int& status) {
    double sq[MAX_POINTS * D], c[D], lo[D], hi[D], s = 0.0;
    int sidx[MAX_POINTS];
    n = n < 0 ? 0 : (n > n_max ? n_max : n);
    int live = 0;
    for (int k = 0; k < D; ++k) {
        lo[k] = __builtin_inf();
        hi[k] = -__builtin_inf();
    }
    for (int i = 0; i < n; ++i) {
        if (!((keep >> i) & 1)) continue;
        for (int k = 0; k < D; ++k) {
            lo[k] = fmin(lo[k], X[(size_t)i * D + k]);
            hi[k] = fmax(hi[k], X[(size_t)i * D + k]);
        }
        sidx[live++] = i;
    }
    for (int k = 0; k < D; ++k) c[k] = centre(lo[k], hi[k]);
    for (int j = 0; j < live; ++j) {
        double p[D];
        for (int k = 0; k < D; ++k) p[k] = X[(size_t)sidx[j] * D + k];
        s = fmax(s, reach<D>(p, c));
    }
    count = 0;
    status = HS_OK;
    if (stageable<D>(s, live)) {
        for (int j = 0; j < live; ++j)
            for (int k = 0; k < D; ++k) sq[j * D + k] = (X[(size_t)sidx[j] * D + k] - c[k]) / s;
        double nu[D], off = 0.0;   // the candidate the list is looking at
        uint64_t w = 0;
        const bool over = wenum::greedy_list<D>(
            live, f_max, count,
            [&](const int(&idx)[D]) {   // (a flat candidate ends the list empty)
                const int kind = candidate<D>(sq, sidx, live, idx, nu, off, w);
                return kind == CAND_FLAT ? wenum::LIST_END : (kind == CAND_FACET ? wenum::LIST_TAKE : wenum::LIST_SKIP);
            },
            [&](const int q) { return same<D>(nu, off, Ao + (size_t)q * D, bo[q]); },
            [&](const int q, const int(&idx)[D]) {
                for (int k = 0; k < D; ++k) {
                    Ao[(size_t)q * D + k] = nu[k];
                    if (basis) basis[(size_t)q * D + k] = sidx[idx[k]];
                }
                bo[q] = off;
                on[q] = w;
            });
        if (over) status = HS_OVERFLOW;
    }
    if (count == 0) status = HS_FLAT;
    for (int q = 0; q < count; ++q) bo[q] = unstage<D>(Ao + (size_t)q * D, bo[q], c, s);
    for (int q = count; q < f_max; ++q) {
        bo[q] = __builtin_nan("");
        on[q] = 0;
        for (int k = 0; k < D; ++k) {
            Ao[(size_t)q * D + k] = __builtin_nan("");
            if (basis) basis[(size_t)q * D + k] = -1;
        }
    }
}

}  // namespace hullenum
}  // namespace plp
