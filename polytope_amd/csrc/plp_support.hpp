// plp_support.hpp -- support functions  h_P(c) = max { c.x : A x <= b }  of a polytope in MANY directions, the rows read
// once: support_kernel<D, RV> (plp_support.hip) behind plp_support_batch.
//
// Every LP of a polytope is   min (-c).x'   s.t.  a_i.x' <= beta_i  (beta_i = b_i - a_i.xc > 0: xc strictly inside),
// x' free, started at x' = 0 -- the LP the one-LP-per-lane engine (plp_lane_lp.hpp: walk3 / walk4) solves for an arbitrary
// cost.  A workgroup (one wavefront) stages the rows of its polytopes into LDS once, as a_i and beta_i, and every lane
// walks one direction of one polytope; K directions of a polytope take L lanes and ceil(K / L) rounds.
//
// Tiles, the LDS layout and the frame of the kernel: plp_row_tile.hpp (one staged scalar per row, beta_i).
//
// Status per (polytope, direction), the contract of bbox_lane_kernel:
//     0  optimum: val = c.x, x = xc + x'
//     3  unbounded in that direction: val = +inf, x = NaN
//     1  NOT SETTLED HERE, handed back to the caller (val = x = NaN): a live row with beta_i <= 0 (xc is not strictly
//        inside), a centre or a direction that is not finite, a walk handed back (ST_RETRY: a run of degenerate steps,
//        dependent active rows, the iteration cap), or a final point that fails one of the two end checks:
//        feasibility  max_i (a_i.x' - beta_i) <= 1e-10 min(max(1, |beta|_max), max(1, |x|_inf))
//                     and  v_i c.x' <= 1e-10 extent beta_i  for every row the point is outside of by v_i > 0,
//        optimality   multipliers lam >= 0 on the rows the walk ended on with  sum lam_j slack_j  and  |c - sum lam_j a_j|_1
//                     below 1e-10 / 1e-12 of the extent max(1, |x|_inf, |c.x|)  (certificate() below).
// What a status 0 guarantees, with E = max(1, |x|_inf, |c.x|) and h* the exact optimum of the rows as staged:
//     h <= h* + 1e-10 E          (the point scaled towards the centre by max_i v_i / beta_i is feasible),
//     h >= h* - 1e-10 E - |r|_1 |y - x'|_inf,   |r|_1 <= 1e-12 E / max(1, |x'|_inf),   y an optimal point:
// the last term is below 1e-10 E for every optimum within 100 max(1, |x'|) of the point, and is NOT bounded for an optimal
// face that reaches further (a residual at rounding level, 1e-16 |c|, needs 1e6 for it).  Before the second check four of
// 2 280 LPs of a `dup` soak seed (rows 1e-9 .. 1e-5 rad apart) came back as status 0 with h = 1.249 for 2.090 and the like;
// scripts/soak_support.py now finds every status 0 of 5.3 M LPs within 1e-9 E of the oracle's h or, on the 53 where the
// oracle itself is off (it reads entries <= 1e-9 as zero), of the exact rational optimum.  The certificate is this file's
// own, in plain doubles on at most four rows; it is not the certificate of plp_verify (LU, refined, every row to
// 2e-14) -- what fails here goes there through resolve=True.
//
// The per-LP function compiles for the host as well (g++, tests/cabi/support_host.cpp), as plp_lane_lp.hpp does: the same
// source, explicit fma and -ffp-contract=off on both sides.
#pragma once
#include <stddef.h>

#include "plp_lane_lp.hpp"
#include "plp_row_tile.hpp"

namespace plp {
namespace support {

constexpr double END_TOL = 1e-10;   // end check, feasibility: relative to min(max(1, |beta|_max), max(1, |x|_inf))
constexpr int MAX_DIM = 4;
// (the tile rules under the names they had here before plp_row_tile.hpp: host restatements written against those still build)
using rowtile::polytopes_per_group, rowtile::row_slots;

// beta_i = b_i - a_i.xc, the sum in column order
template <int D>
PLP_LANE_FN double beta_of(const double* a, const double bi, const double* xc) {
    double s = a[0] * xc[0];
#pragma unroll
    for (int k = 1; k < D; ++k) s = fma(a[k], xc[k], s);
    return bi - s;
}

// lam = argmin | v - sum_j lam_j n_j |_2 over the first `nact` of four rows (the others are zero rows and get lam_j = 0):
// Gram-Schmidt without square roots, q_j = n_j - sum_{i<j} mu_ji q_i, then back substitution.  Every index is a compile-time
// one (registers).  Rows that are dependent to working precision give q_j.q_j = 0 and a lam that is not a number: the
// certificate below then fails, which is the answer for such a basis.
PLP_LANE_FN void ls_multipliers(const double (&n)[4][4], const int nact, const double (&v)[4], double (&lam)[4]) {
    double q[4][4], mu[4][4], qq[4], g[4];
    double r[4] = {v[0], v[1], v[2], v[3]};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
#pragma unroll
        for (int k = 0; k < 4; ++k) q[j][k] = n[j][k];
#pragma unroll
        for (int i = 0; i < j; ++i) {
            mu[j][i] = lane::dot4(q[j][0], q[j][1], q[j][2], q[j][3], q[i][0], q[i][1], q[i][2], q[i][3]) / qq[i];
#pragma unroll
            for (int k = 0; k < 4; ++k) q[j][k] = fma(-mu[j][i], q[i][k], q[j][k]);
        }
        const double s = lane::dot4(q[j][0], q[j][1], q[j][2], q[j][3], q[j][0], q[j][1], q[j][2], q[j][3]);
        qq[j] = j < nact ? s : 1.0;
        g[j] = lane::dot4(r[0], r[1], r[2], r[3], q[j][0], q[j][1], q[j][2], q[j][3]) / qq[j];
#pragma unroll
        for (int k = 0; k < 4; ++k) r[k] = fma(-g[j], q[j][k], r[k]);
    }
#pragma unroll
    for (int j = 3; j >= 0; --j) {
        double s = g[j];
#pragma unroll
        for (int i = j + 1; i < 4; ++i) s = fma(-mu[i][j], lam[i], s);
        lam[j] = s;
    }
}

// The optimality certificate of a point x' with value c.x' on `nact` active rows n_j (slacks sl_j = beta_j - n_j.x'):
// multipliers lam >= 0 with  r = c - sum lam_j n_j.  Every feasible y has
//     c.y  =  sum lam_j n_j.y + r.y  <=  sum lam_j beta_j + r.y  =  c.x' + sum lam_j sl_j - r.x' + r.y,
// so a FEASIBLE x' is optimal to  gap + |r|_1 |y - x'|_inf,  gap = sum lam_j |sl_j|  (what an x' a little outside a row
// overshoots by is the feasibility check's business, solve_one).  The bound holds for ANY lam >= 0, however it was computed; r and gap are plain sums of a few products (rounding 1e-16 |c|).  So nothing here trusts the walk's own
// multipliers (on rows 1e-9 .. 1e-5 rad apart, Gram determinants of 1e-18 .. 1e-10, their signs are rounding), nor the
// solve below: a bad lam shows as a residual and the LP is handed back.  lam: least squares on the rows (exact for a
// vertex), one round of refinement, negative entries -- rounding at a degenerate vertex, or a row the walk should have
// left -- replaced by zero before r is formed.
//     gap <= OPT_TOL_GAP scale,   |r|_1 max(1, |x'|_inf) <= OPT_TOL_RES scale,   scale = max(1, |x|_inf, |c.x|)
// (the extent the support tests measure h against; |y - x'| is TAKEN as the walk's own reach, max(1, |x'|): an assumption, not
// a bound -- see the guarantee in the header).  A residual
// is all rounding or a direction the walk did not follow, so its bound is the tighter one; the walk's own stop, a projected
// cost below LANE_TOL_D |c|, passes it for |c|_1 <= 0.1 / max(1, |x'|_inf).
constexpr double OPT_TOL_GAP = 1e-10, OPT_TOL_RES = 1e-12;

PLP_LANE_FN bool certificate(const double (&n)[4][4], const int nact, const double (&c)[4], const double (&sl)[4],
                             const double xpn, const double scale0) {
    double lam[4], dl[4], r[4];
    ls_multipliers(n, nact, c, lam);
#pragma unroll
    for (int k = 0; k < 4; ++k) r[k] = fma(-lam[3], n[3][k], fma(-lam[2], n[2][k], fma(-lam[1], n[1][k], fma(-lam[0], n[0][k], c[k]))));
    ls_multipliers(n, nact, r, dl);
    double gap = 0.0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        lam[j] = lam[j] + dl[j];
        lam[j] = lam[j] > 0.0 ? lam[j] : (lam[j] <= 0.0 ? 0.0 : lam[j]);   // (a NaN stays)
        gap = fma(lam[j], fabs(sl[j]), gap);
    }
    double r1 = 0.0;
#pragma unroll
    for (int k = 0; k < 4; ++k)
        r1 += fabs(fma(-lam[3], n[3][k], fma(-lam[2], n[2][k], fma(-lam[1], n[1][k], fma(-lam[0], n[0][k], c[k])))));
    return (gap <= OPT_TOL_GAP * scale0) & (r1 * xpn <= OPT_TOL_RES * scale0);
}

// One direction of one polytope.  pA / pbeta: the polytope's staged rows -- element (i, k) at pA[(i * D + k) * LS],
// beta_i at pbeta[i * LS], RV row slots, rows i >= m zero with beta = 0.  c: the direction (columns >= D zero), xc the
// interior point.  `go` = false: the lane has no LP (it still takes part in the wavefront's votes).
// ANY(pred): true while any lane of the wavefront still runs (device: __any; host: the predicate itself).
template <int D, int RV, class AnyF>
PLP_LANE_FN void solve_one(const double* pA, const double* pbeta, const int LS, const int m, const double (&c)[4],
                           const double (&xc)[4], const bool go, AnyF ANY, double& val, double (&x)[4], int& status) {
    static_assert(D >= 1 && D <= MAX_DIM, "the lane engine walks in R^3 (lower dimensions are embedded) or R^4");
    auto row_of = [&](const int i, double& a0, double& a1, double& a2, double& a3) {
        const double* base = pA + (size_t)(i * D) * LS;
        a0 = base[0];
        a1 = D > 1 ? base[(D > 1 ? 1 : 0) * LS] : 0.0;
        a2 = D > 2 ? base[(D > 2 ? 2 : 0) * LS] : 0.0;
        a3 = D > 3 ? base[(D > 3 ? 3 : 0) * LS] : 0.0;
    };
    // a live row the centre does not clear (NaN included): nothing starts from this centre
    bool inside = true;
    double bmax = 0.0;
#pragma unroll 4
    for (int i = 0; i < RV; ++i) {
        const double beta = pbeta[i * LS];
        inside = inside & ((i >= m) | (beta > 0.0));
        bmax = fmax(bmax, fabs(beta));
    }
#pragma unroll
    for (int k = 0; k < D; ++k)   // (a polytope without rows: the centre still has to be a point; the direction a vector)
        inside = inside & (xc[k] - xc[k] == 0.0) & (c[k] - c[k] == 0.0);
    const bool run = go & inside;
    double xp[4] = {0.0, 0.0, 0.0, 0.0};
    int wst, nact, w[4] = {-1, -1, -1, -1};   // how the walk ended, and on which rows
    if constexpr (D == 4) {
        lane::Lp4 S;
        lane::walk4(
            S, -c[0], -c[1], -c[2], -c[3], run,
            [&](int i, double& a0, double& a1, double& a2, double& a3) { row_of(i, a0, a1, a2, a3); },
            [&](double d0, double d1, double d2, double d3, double x0, double x1, double x2, double x3, double tolp, double& bs,
                double& bd, int& bi) {
#pragma unroll 4
                for (int i = 0; i < RV; ++i) {
                    double a0, a1, a2, a3;
                    row_of(i, a0, a1, a2, a3);
                    lane::ratio_row4(a0, a1, a2, a3, pbeta[i * LS], i, d0, d1, d2, d3, x0, x1, x2, x3, tolp, bs, bd, bi);
                }
            },
            ANY);
        xp[0] = S.x0; xp[1] = S.x1; xp[2] = S.x2; xp[3] = S.x3;
        w[0] = S.w0; w[1] = S.w1; w[2] = S.w2; w[3] = S.w3;
        nact = S.nact;
        wst = S.status;
    } else {
        lane::Lp3 S;
        lane::walk3(
            S, -c[0], -c[1], -c[2], run,
            [&](int i, double& a0, double& a1, double& a2) {
                double a3;
                row_of(i, a0, a1, a2, a3);
            },
            [&](double d0, double d1, double d2, double x0, double x1, double x2, double tolp, double& bs, double& bd, int& bi) {
#pragma unroll 4
                for (int i = 0; i < RV; ++i) {
                    double a0, a1, a2, a3;
                    row_of(i, a0, a1, a2, a3);
                    lane::ratio_row(a0, a1, a2, pbeta[i * LS], i, d0, d1, d2, x0, x1, x2, tolp, bs, bd, bi);
                }
            },
            [&](double d0, double d1, double d2, double tolp, double& bs, double& bd, int& bi) {
#pragma unroll 4
                for (int i = 0; i < RV; ++i) {
                    double a0, a1, a2, a3;
                    row_of(i, a0, a1, a2, a3);
                    lane::ratio_row0(a0, a1, a2, pbeta[i * LS], i, d0, d1, d2, tolp, bs, bd, bi);
                }
            },
            ANY);
        xp[0] = S.x0; xp[1] = S.x1; xp[2] = S.x2;
        w[0] = S.w0; w[1] = S.w1; w[2] = S.w2;
        nact = S.nact;
        wst = S.status;
    }
    // the extent the answer is measured against: max(1, |x|_inf, |c.x|)
    double xn = 1.0, xpn = 1.0, cx = 0.0;
#pragma unroll
    for (int k = 0; k < D; ++k) {
        const double xk = xc[k] + xp[k];
        xn = fmax(xn, fabs(xk));
        xpn = fmax(xpn, fabs(xp[k]));
        cx = k == 0 ? c[0] * xk : fma(c[k], xk, cx);
    }
    // end check 1, feasibility: the point the walk stopped on against every row once more (a NaN fails it).  At a vertex the
    // walk looks at multipliers only: a row it stands beyond -- the twin of an active row, tilted by 1e-9 -- is seen here or not
    // at all.  What a violation v_i = a_i.x' - beta_i > 0 is worth: (1 - s) x' with s = max_i v_i / beta_i is feasible (the centre
    // x' = 0 clears row i by beta_i), so the value c.x' overshoots the optimum by at most s c.x'; that is held below
    // OPT_TOL_GAP of the extent, whatever the angle between the rows.
    const double tol = END_TOL * fmin(fmax(1.0, bmax), xn);
    const double over = OPT_TOL_GAP * fmax(xn, fabs(cx));
    double cxp = 0.0;
#pragma unroll
    for (int k = 0; k < D; ++k) cxp = fma(c[k], xp[k], cxp);
    cxp = fabs(cxp);
    bool feas = true;
#pragma unroll 4
    for (int i = 0; i < RV; ++i) {
        double a0, a1, a2, a3;
        row_of(i, a0, a1, a2, a3);
        const double ax = D == 4 ? lane::dot4(a0, a1, a2, a3, xp[0], xp[1], xp[2], xp[3]) : lane::dot3(a0, a1, a2, xp[0], xp[1], xp[2]);
        const double beta = pbeta[i * LS], v = ax - beta;
        feas = feas & (v <= tol) & (v * cxp <= over * beta);
    }
    // end check 2, optimality: the rows the walk ended on must carry a dual certificate at that point
    bool opt = false;
    if (ANY(run & (wst == ST_OPT))) {
        double n[4][4], sl[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const bool on = (j < nact) & (w[j] >= 0) & (w[j] < RV);
            const int i = on ? w[j] : 0;
            double a0, a1, a2, a3;
            row_of(i, a0, a1, a2, a3);
            n[j][0] = on ? a0 : 0.0; n[j][1] = on ? a1 : 0.0; n[j][2] = on ? a2 : 0.0; n[j][3] = on ? a3 : 0.0;
            sl[j] = on ? pbeta[i * LS] - lane::dot4(a0, a1, a2, a3, xp[0], xp[1], xp[2], xp[3]) : 0.0;
        }
        opt = certificate(n, nact, c, sl, xpn, fmax(xn, fabs(cx)));
    }
    status = !run ? 1 : (wst == ST_OPT ? (feas & opt ? 0 : 1) : (wst == ST_UNBND ? 3 : 1));
    const double qnan = __builtin_nan("");
    double v = 0.0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const double xk = k < D ? xc[k] + xp[k] : 0.0;
        x[k] = status == 0 ? xk : qnan;
        if (k < D) v = k == 0 ? c[0] * xk : fma(c[k], xk, v);
    }
    val = status == 0 ? v : (status == 3 ? __builtin_inf() : qnan);
}

}  // namespace support
}  // namespace plp
