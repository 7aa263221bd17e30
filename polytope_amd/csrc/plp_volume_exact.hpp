// plp_volume_exact.hpp -- the exact volume and the facet areas of a small polytope {A x <= b} (d <= 4, at most 64 rows) by
// Lasserre's facet recursion on the rows: volume_exact_kernel<D> (plp_volume_exact.hip) behind plp_vol_exact_batch.
//
//     vol_D(P) = (1 / D) sum_i h_i vol_{D-1}(P ^ H_i),     h_i the signed distance of the reference point from row i,
//
// taken down to lines, where the measure is the length of an interval (min / max over the other rows).  No vertex list and
// no LP; every term is continuous in the data, and a row that does not touch a face adds an interval of length 0.
//
// The contract, as a sequential rule (volume_exact::one<D> below is that rule; the kernel evaluates the same terms 64 at a
// time and adds them in the same order):
//   staging   the live rows (i < m, bit i of `keep`) in increasing row index, each scaled to unit 2-norm u_i = a_i / |a_i|
//             (wenum::unit_row).  A live zero row is not staged: with b_i >= 0 it says nothing, with b_i < 0 (or NaN) the
//             member is VS_EMPTY with volume 0.  Then beta_i = ((b_i - a_i.c) / |a_i|) / s with c = xc (0 when absent) and
//             s = scale (1 when absent): the rows of (P - c) / s.  (b_i / |a_i| - u_i.c is the same number with one more
//             rounding at the size of the offset: 1e-13 of the volume at |c| = 1e3.)  All tolerances are absolute on
//             these rows.
//   chains    a chain (i_1 .. i_k), k <= D - 1, of distinct staged rows carries orthonormal q_1 .. q_k, distances h_1 .. h_k
//             and foot points p_0 = 0, p_l = p_{l-1} + h_l q_l: the point of the flat {row i_1 .. i_l tight} nearest p_{l-1}.
//             A staged row j outside the chain is projected level by level: w_0 = u_j, s_0 = 1,
//             w_l = w_{l-1} - (w_{l-1}.q_l) q_l, s_l = |w_l|^2.
//   parallel  j is parallel at the first level l with |w_l| <= PAR_TOL |w_{l-1}|: the sine of the angle between w_{l-1} and
//             the chain row's own projection v_{l-1} (q_l = v_{l-1} / |v_{l-1}|).  It is tested as
//             |w ^ v|^2 <= PAR_TOL^2 |w|^2 |v|^2, the wedge product by its 2 x 2 minors: the same bits whichever of the two
//             rows is in the chain.  (Tested on |w_l| itself, two rows 1e-12 rad apart can each find the other live, or
//             each find the other parallel, by rounding: a facet then counts twice or not at all.)
//             Then rho = (beta_j - u_j.p_l) / |w_{l-1}|, and
//               rho < -RES_TOL                                          the chain's face is empty (a kill);
//               |rho| <= RES_TOL, w_{l-1}.q_l > 0 and j < i_l           a kill too: two rows induce one face of the flat, and
//                                                                       the one of lower index owns it;
//               otherwise                                               j says nothing on this chain.
//             A kill at level l depends on the prefix (i_1 .. i_l) alone.
//   live      a row that is parallel at no level is live on the chain: induced normal w_k, r = beta_j - u_j.p_k.  It extends
//             the chain by q_{k+1} = w_k / |w_k|, h_{k+1} = r / |w_k|.
//   lines     a full chain (k = D - 1) is a line through p_k with direction t orthogonal to q_1 .. q_k: t = 1 (D = 1),
//             (-q_1[1], q_1[0]) (D = 2), q_1 x q_2 (D = 3), the generalised cross product of q_1, q_2, q_3 expanded along its
//             first row (D = 4; line_dir below).  Over the live rows, sigma = w_k.t:  sigma > 0: hi = min(hi, r / sigma),
//             sigma < 0: lo = max(lo, r / sigma).  Its measure is hi - lo where that is positive (+inf without an end), else 0.
//   sums      the measure of a chain of flat dimension e >= 2 that is not killed: +inf when it has no live row (the whole
//             flat lies in P), else the sum over its live rows j IN INCREASING INDEX of (h_j / e) measure(chain + j), +inf
//             as soon as one of those measures is.  A killed chain measures +0.
//   outputs   volume = s^D measure(()); area[i] = s^(D-1) measure((i)) at the ORIGINAL row index, 0 for a row that is not
//             staged (for D = 1: 1 for the lowest-index row that attains each end of a non-empty interval); status VS_OK
//             (a volume of 0 is the answer for an empty or flat set), VS_UNBOUNDED (volume +inf: some chain has no end or no
//             live row, which includes a member without rows), VS_EMPTY (an infeasible zero row: volume 0, areas 0).
//             VS_FLAT is set by callers that test for it first (volume_exact_batch of the Python package).
//
// How the rule is evaluated, on both sides: every tuple (i_1 .. i_{D-1}) of staged rows, repeats included, is one term
// (tuple_term): its longest valid prefix is built (a row that repeats, or is not live on the rows before it, ends the
// prefix), ONE pass over the staged rows finds kills, counts live rows and, on a full chain, cuts the line.  The term is 0
// when a kill was found, +inf when there is no live row, 0 when the prefix is not full (the tuples that extend the prefix by
// a live row carry its measure), else (h_{D-1} / 2) times the length.  The sums over the last index, then the one before it
// and so on, in increasing index, are the rule's sums: the terms of rows that are not live are +0 and change no bit of a
// sum that starts at +0.
//
// Why these tolerances.  PAR_TOL = 1e-12: rows this close in direction are one row twice (extreme::DET_TOL); a wider
// threshold drops rows that still cut (measured: 1e-9 loses 3.5 % of a volume at d = 4), and a second test for near
// duplicates loses up to 15 % for rows 1e-11 .. 1e-9 rad apart, so there is one threshold and no dedupe.  RES_TOL = 1e-9 on
// the scaled rows: extreme::FEAS_TOL, the distance below which two parallel rows are the same face.
//
// The same source compiles for the host (g++ -ffp-contract=off, tests/cabi/volume_exact_host.cpp): sums of products are
// separate multiplies and adds in a fixed order, sqrt and / are correctly rounded on both sides, min / max are written as
// comparisons, so the device's numbers are the host's bit for bit.
#pragma once
#include "plp_enum.hpp"

namespace plp {
namespace volume_exact {

using wenum::dot;
constexpr int MAX_DIM = wenum::MAX_DIM, MAX_ROWS = wenum::MAX_ITEMS;
constexpr double PAR_TOL = 1e-12, PAR_TOL2 = PAR_TOL * PAR_TOL, RES_TOL = 1e-9;
enum : int { VS_OK = 0, VS_UNBOUNDED = 1, VS_EMPTY = 2, VS_FLAT = 3 };   // include/plp.h: PLP_VS_*

// the row stride of the term table of n staged rows (odd: the lanes that add its rows read different LDS banks)
PLP_ENUM_FN int tab_stride(const int n) { return n | 1; }
// LDS (or host scratch) of one polytope: the staged rows [m_max][D] and their beta, the facet terms and facet measures
// [m_max] each, and for D >= 3 the term table [m_max][tab_stride(m_max)] of the last two chain levels
constexpr size_t lds_bytes(int D, int m_max) {
    return ((size_t)m_max * (D + 3) + (D >= 3 ? (size_t)m_max * (m_max | 1) : 0)) * sizeof(double);
}

PLP_ENUM_FN double inf() { return __builtin_inf(); }

// (h / e) R, +inf when R is
PLP_ENUM_FN double weigh(const double h, const int e, const double R) { return R == inf() ? inf() : (h / (double)e) * R; }

// one input row -> its staged form on the rows of (P - c) / s (wenum::unit_row and its verdict, beta shifted and scaled)
template <int D>
PLP_ENUM_FN int stage_row(const double (&a)[D], const double bi, const bool shifted, const double (&c)[D], const double s,
                          double (&u)[D], double& beta) {
    double nrm;
    const int kind = wenum::unit_row<D>(a, bi, u, nrm);
    if (kind == 1) beta = ((bi - (shifted ? dot<D>(a, c) : 0.0)) / nrm) / s;
    return kind;
}

// the chain of a tuple: K = D - 1 levels at the most, v of them valid (arrays of at least one level, so that D = 1 compiles)
template <int D>
struct Chain {
    static constexpr int K = D > 1 ? D - 1 : 1;
    double q[K][D], p[K][D], h[K];
    double vr[K][D], vs[K];   // the chain rows' own projections, not normalised, and their squared norms
    int idx[K], v;
};

// row j = (u, beta) against the first `upto` levels of the chain -> 0 live (w = w_upto, s2 = |w|^2), 1 says nothing, 2 kill
template <int D>
PLP_ENUM_FN int classify(const Chain<D>& c, const int upto, const double (&u)[D], const double beta, const int j, double (&w)[D],
                         double& s2) {
#pragma unroll
    for (int k = 0; k < D; ++k) w[k] = u[k];
    double sprev = 1.0;
    int res = 0;
#pragma unroll
    for (int l = 0; l < D - 1; ++l) {
        if (l < upto && res == 0) {
            const double g = dot<D>(w, c.q[l]);
            double w2[D], wedge = 0.0;
#pragma unroll
            for (int a = 0; a < D; ++a) {
                w2[a] = w[a] - g * c.q[l][a];
#pragma unroll
                for (int e = a + 1; e < D; ++e) {
                    const double mn = w[a] * c.vr[l][e] - w[e] * c.vr[l][a];
                    wedge = wedge + mn * mn;
                }
            }
            const double sl = dot<D>(w2, w2);
            if (wedge <= PAR_TOL2 * (sprev * c.vs[l])) {
                const double rho = (beta - dot<D>(u, c.p[l])) / sqrt(sprev);
                const bool kill = rho < -RES_TOL || (fabs(rho) <= RES_TOL && g > 0.0 && j < c.idx[l]);
                res = kill ? 2 : 1;
            } else {
#pragma unroll
                for (int k = 0; k < D; ++k) w[k] = w2[k];
                sprev = sl;
            }
        }
    }
    s2 = sprev;
    return res;
}

// r = beta - u.p_v of a row on a chain with v valid levels
template <int D>
PLP_ENUM_FN double residual(const Chain<D>& c, const double (&u)[D], const double beta) {
    double r = beta;
#pragma unroll
    for (int l = 0; l < D - 1; ++l)
        if (l + 1 == c.v) r = beta - dot<D>(u, c.p[l]);
    return r;
}

// the longest valid prefix of the tuple idx[0 .. levels) on the staged rows sU[n][D], sb[n]; h beyond it is 0
template <int D>
PLP_ENUM_FN void build(const double* sU, const double* sb, const int (&idx)[Chain<D>::K], const int levels, Chain<D>& c) {
    c.v = 0;
#pragma unroll
    for (int l = 0; l < Chain<D>::K; ++l) {
        c.h[l] = c.vs[l] = 0.0;
        c.idx[l] = -1;
#pragma unroll
        for (int k = 0; k < D; ++k) c.q[l][k] = c.p[l][k] = c.vr[l][k] = 0.0;
    }
#pragma unroll
    for (int l = 0; l < D - 1; ++l) {
        if (l < levels && c.v == l) {
            const int j = idx[l];
            bool fresh = true;
#pragma unroll
            for (int e = 0; e < D - 1; ++e) fresh = fresh & !(e < l && c.idx[e] == j);
            if (fresh) {
                double u[D], w[D], s2;
#pragma unroll
                for (int k = 0; k < D; ++k) u[k] = sU[j * D + k];
                if (classify<D>(c, l, u, sb[j], j, w, s2) == 0) {
                    const double nk = sqrt(s2), r = residual<D>(c, u, sb[j]);
                    c.h[l] = r / nk;
                    c.vs[l] = s2;
#pragma unroll
                    for (int k = 0; k < D; ++k) {
                        c.vr[l][k] = w[k];
                        c.q[l][k] = w[k] / nk;
                        c.p[l][k] = (l > 0 ? c.p[l > 0 ? l - 1 : 0][k] : 0.0) + c.h[l] * c.q[l][k];
                    }
                    c.idx[l] = j;
                    c.v = l + 1;
                }
            }
        }
    }
}

// the direction of the line of a full chain
template <int D>
PLP_ENUM_FN void line_dir(const Chain<D>& c, double (&t)[D]) {
    if constexpr (D == 1) {
        t[0] = 1.0;
    } else if constexpr (D == 2) {
        t[0] = -c.q[0][1];
        t[1] = c.q[0][0];
    } else if constexpr (D == 3) {
        const double(&a)[3] = c.q[0];
        const double(&b)[3] = c.q[1];
        t[0] = a[1] * b[2] - a[2] * b[1];
        t[1] = a[2] * b[0] - a[0] * b[2];
        t[2] = a[0] * b[1] - a[1] * b[0];
    } else {
        const double(&a)[4] = c.q[0];
        const double(&b)[4] = c.q[1];
        const double(&g)[4] = c.q[2];
        // the 2 x 2 minors of rows b, g, then the cofactors of the first row of [e; a; b; g]
        const double m01 = b[0] * g[1] - b[1] * g[0], m02 = b[0] * g[2] - b[2] * g[0], m03 = b[0] * g[3] - b[3] * g[0];
        const double m12 = b[1] * g[2] - b[2] * g[1], m13 = b[1] * g[3] - b[3] * g[1], m23 = b[2] * g[3] - b[3] * g[2];
        t[0] = (a[1] * m23 - a[2] * m13) + a[3] * m12;
        t[1] = -((a[0] * m23 - a[2] * m03) + a[3] * m02);
        t[2] = (a[0] * m13 - a[1] * m03) + a[3] * m01;
        t[3] = -((a[0] * m12 - a[1] * m02) + a[2] * m01);
    }
}

// The term of the tuple idx (D >= 2): see the head of this file.  `len` is the measure of the tuple's line (the facet area
// for D = 2), 0 / +inf as the term.
template <int D>
PLP_ENUM_FN double tuple_term(const double* sU, const double* sb, const int n, const int (&idx)[Chain<D>::K], double& len) {
    Chain<D> c;
    build<D>(sU, sb, idx, D - 1, c);
    const bool full = c.v == D - 1;
    double t[D];
    line_dir<D>(c, t);
    double lo = -inf(), hi = inf();
    bool killed = false;
    int nlive = 0;
    for (int j = 0; j < n; ++j) {
        bool in_chain = false;
#pragma unroll
        for (int l = 0; l < D - 1; ++l) in_chain = in_chain | (c.idx[l] == j);   // (idx beyond v is -1)
        if (in_chain) continue;
        double u[D], w[D], s2;
#pragma unroll
        for (int k = 0; k < D; ++k) u[k] = sU[j * D + k];
        const double beta = sb[j];
        const int cls = classify<D>(c, c.v, u, beta, j, w, s2);
        killed = killed | (cls == 2);
        if (cls != 0) continue;
        ++nlive;
        if (full) {
            const double sigma = dot<D>(w, t), x = residual<D>(c, u, beta) / sigma;
            if (sigma > 0.0) hi = x < hi ? x : hi;
            if (sigma < 0.0) lo = x > lo ? x : lo;
        }
    }
    if (killed) return len = 0.0;
    if (nlive == 0) return len = inf();
    if (!full) return len = 0.0;
    const double span = hi - lo;
    len = span > 0.0 ? span : 0.0;
    return weigh(c.h[D - 2 >= 0 ? D - 2 : 0], 2, len);
}

// h_l of the prefix idx[0 .. l] (0 where it is not valid): the weight of the sums above the table
template <int D>
PLP_ENUM_FN double prefix_h(const double* sU, const double* sb, const int (&idx)[Chain<D>::K], const int l) {
    Chain<D> c;
    build<D>(sU, sb, idx, l + 1, c);
    double h = 0.0;
#pragma unroll
    for (int e = 0; e < D - 1; ++e)
        if (e == l) h = c.h[e];
    return h;
}

// D = 1 on the staged rows: the interval, and the rows that own its ends (-1: none)
PLP_ENUM_FN double interval(const double* sU, const double* sb, const int n, int& own_lo, int& own_hi) {
    double lo = -inf(), hi = inf();
    own_lo = own_hi = -1;
    for (int j = 0; j < n; ++j) {
        const double x = sb[j] / sU[j];
        if (sU[j] > 0.0 && x < hi) { hi = x; own_hi = j; }
        if (sU[j] < 0.0 && x > lo) { lo = x; own_lo = j; }
    }
    if (!(hi >= lo)) own_lo = own_hi = -1;
    const double span = hi - lo;
    return span > 0.0 ? span : 0.0;
}

// s^k by repeated multiplication
PLP_ENUM_FN double power(const double s, const int k) {
    double r = 1.0;
    for (int e = 0; e < k; ++e) r = r * s;
    return r;
}

// The whole rule for one polytope, sequentially (the host build; the kernel's answers are held against it bit for bit).
// A[m_max][D], b[m_max], m rows of them in use, keep: bit i = row i is live; xc[D] or nullptr, scale; area[m_max] or nullptr.
// work: lds_bytes(D, m_max) bytes.
template <int D>
PLP_ENUM_FN void one(const int m_max, const double* A, const double* b, int m, const uint64_t keep, const double* xc,
                     const double scale, double& volume, double* area, int& status, double* work) {
    double* sU = work;
    double* sb = sU + (size_t)m_max * D;
    double* fterm = sb + m_max;    // the facets' terms of the volume
    double* fmeas = fterm + m_max;   // the facets' measures
    double* tab = fmeas + m_max;
    int sidx[MAX_ROWS];
    m = m < 0 ? 0 : (m > m_max ? m_max : m);
    int n = 0;
    bool empty = false;
    for (int i = 0; i < m; ++i) {
        if (!((keep >> i) & 1)) continue;
        double a[D], c[D], u[D], beta;
        for (int k = 0; k < D; ++k) {
            a[k] = A[(size_t)i * D + k];
            c[k] = xc ? xc[k] : 0.0;
        }
        const int kind = stage_row<D>(a, b[i], xc != nullptr, c, scale, u, beta);
        empty = empty | (kind == 2);
        if (kind != 1) continue;
        for (int k = 0; k < D; ++k) sU[n * D + k] = u[k];
        sb[n] = beta;
        sidx[n++] = i;
    }
    if (area)
        for (int i = 0; i < m_max; ++i) area[i] = 0.0;
    if (empty) {
        volume = 0.0;
        status = VS_EMPTY;
        return;
    }
    double vol = 0.0;
    if (n == 0) {
        vol = inf();
    } else if constexpr (D == 1) {
        int own_lo, own_hi;
        vol = interval(sU, sb, n, own_lo, own_hi);
        fmeas[0] = 0.0;
        if (area && own_lo >= 0) area[sidx[own_lo]] = 1.0;
        if (area && own_hi >= 0) area[sidx[own_hi]] = 1.0;
    } else if constexpr (D == 2) {
        for (int i1 = 0; i1 < n; ++i1) {
            const int idx[1] = {i1};
            fterm[i1] = tuple_term<2>(sU, sb, n, idx, fmeas[i1]);
        }
        for (int i1 = 0; i1 < n; ++i1) vol = vol + fterm[i1];
    } else {
        const int ns = tab_stride(n);
        const int outer = D == 4 ? n : 1;
        for (int o = 0; o < outer; ++o) {
            for (int a = 0; a < n; ++a)
                for (int c = 0; c < n; ++c) {
                    int idx[Chain<D>::K];
                    double len;
                    if constexpr (D == 3) { idx[0] = a; idx[1] = c; } else { idx[0] = o; idx[1] = a; idx[2] = c; }
                    tab[a * ns + c] = tuple_term<D>(sU, sb, n, idx, len);
                }
            for (int a = 0; a < n; ++a) {   // the table's rows
                double s = 0.0;
                for (int c = 0; c < n; ++c) s = s + tab[a * ns + c];
                if constexpr (D == 3) {
                    fmeas[a] = s;
                } else {
                    int idx[Chain<D>::K] = {o, a, 0};
                    tab[a * ns] = weigh(prefix_h<D>(sU, sb, idx, 1), 3, s);
                }
            }
            if constexpr (D == 4) {
                double s = 0.0;
                for (int a = 0; a < n; ++a) s = s + tab[a * ns];
                fmeas[o] = s;
            }
        }
        for (int i1 = 0; i1 < n; ++i1) vol = vol + weigh(sb[i1], D, fmeas[i1]);
    }
    volume = vol == inf() ? vol : power(scale, D) * vol;
    status = vol == inf() ? VS_UNBOUNDED : VS_OK;
    if (area && D > 1) {
        const double sa = power(scale, D - 1);
        for (int i1 = 0; i1 < n; ++i1) area[sidx[i1]] = fmeas[i1] == inf() ? fmeas[i1] : sa * fmeas[i1];
    }
}

}  // namespace volume_exact
}  // namespace plp
