// plp_support.hpp -- support functions  h_P(c) = max { c.x : A x <= b }  of a polytope in MANY directions, the rows read
// once: support_kernel<D, RV> (plp_support.hip) behind plp_support_batch.
//
// Every LP of a polytope is   min (-c).x'   s.t.  a_i.x' <= beta_i  (beta_i = b_i - a_i.xc > 0: xc strictly inside),
// x' free, started at x' = 0 -- the LP the one-LP-per-lane engine (plp_lane_lp.hpp: walk3 / walk4) solves for an arbitrary
// cost.  A workgroup (one wavefront) stages the rows of its polytopes into LDS once, as a_i and beta_i, and every lane
// walks one direction of one polytope; K directions of a polytope take L lanes and ceil(K / L) rounds.
//
// Tiles.  L = min(64, next power of two >= K) lanes per polytope would put 64 / L polytopes on the wavefront; the rows of
// NP polytopes take NP * RV * (D + 1) * 8 bytes of LDS, so NP is capped per RV (and L raised to 64 / NP, the extra lanes
// idle) at a footprint that leaves room for four workgroups on a CU's 160 KiB:
//
//     RV (row slots)   polytopes per workgroup, at most   LDS at the cap, D = 3 / D = 4   workgroups per CU by LDS
//         16                     64                              32 KiB / 40 KiB                     5 / 4
//         32                     32                              32 KiB / 40 KiB                     5 / 4
//         64                     16                              32 KiB / 40 KiB                     5 / 4
//
// (K >= 33: one polytope per workgroup, 0.5 .. 2.5 KiB.)  LDS layout: POLYTOPE-INTERLEAVED as in plp_reduce_lane.hpp --
// element (row i, column k) of the tile's polytope p at sA[(i * D + k) * NP + p], beta_i at sbeta[i * NP + p].  The lanes
// of one polytope read one address (a broadcast); lanes of different polytopes read consecutive doubles: within a
// 32-lane half at most 32 of them, 256 bytes = every bank once.
//
// Status per (polytope, direction), the contract of bbox_lane_kernel:
//     0  optimum: val = c.x, x = xc + x'
//     3  unbounded in that direction: val = +inf, x = NaN
//     1  NOT SETTLED HERE, handed back to the caller (val = x = NaN): a live row with beta_i <= 0 (xc is not strictly
//        inside), a centre or a direction that is not finite, a walk handed back (ST_RETRY: a run of degenerate steps,
//        dependent active rows, the iteration cap), or a final point that fails the end check
//        max_i (a_i.x' - beta_i) <= 1e-9 max(1, |beta|_max).
// The end check is feasibility only; optimality is the walk's own multiplier test.  These answers are NOT under the
// certificate of plp_verify.
//
// The per-LP function compiles for the host as well (g++, tests/cabi/support_host.cpp), as plp_lane_lp.hpp does: the same
// source, explicit fma and -ffp-contract=off on both sides.
#pragma once
#include <stddef.h>

#include "plp_lane_lp.hpp"

namespace plp {
namespace support {

constexpr double END_TOL = 1e-9;   // end check, relative to max(1, |beta|_max)
constexpr int MAX_DIM = 4, MAX_ROWS = 64;

// row slots for polytopes of up to m_max rows (0: not taken)
constexpr int row_slots(int m_max) { return m_max < 0 || m_max > MAX_ROWS ? 0 : (m_max <= 16 ? 16 : (m_max <= 32 ? 32 : 64)); }
// polytopes per workgroup at most (the table above)
constexpr int np_cap(int rv) { return 1024 / rv; }
// polytopes per workgroup for K directions: 64 / L, capped; each gets 64 / NP lanes
constexpr int polytopes_per_group(int K, int rv) {
    int L = 1;
    while (L < 64 && L < K) L <<= 1;
    return 64 / L < np_cap(rv) ? 64 / L : np_cap(rv);
}
constexpr size_t lds_bytes(int D, int rv, int np) { return (size_t)np * rv * (D + 1) * sizeof(double); }

// beta_i = b_i - a_i.xc, the sum in column order
template <int D>
PLP_LANE_FN double beta_of(const double* a, const double bi, const double* xc) {
    double s = a[0] * xc[0];
#pragma unroll
    for (int k = 1; k < D; ++k) s = fma(a[k], xc[k], s);
    return bi - s;
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
    int wst;
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
        wst = S.status;
    }
    // end check: the point the walk stopped on against every row once more (a NaN fails it)
    const double tol = END_TOL * fmax(1.0, bmax);
    bool feas = true;
#pragma unroll 4
    for (int i = 0; i < RV; ++i) {
        double a0, a1, a2, a3;
        row_of(i, a0, a1, a2, a3);
        const double ax = D == 4 ? lane::dot4(a0, a1, a2, a3, xp[0], xp[1], xp[2], xp[3]) : lane::dot3(a0, a1, a2, xp[0], xp[1], xp[2]);
        feas = feas & (ax - pbeta[i * LS] <= tol);
    }
    status = !run ? 1 : (wst == ST_OPT ? (feas ? 0 : 1) : (wst == ST_UNBND ? 3 : 1));
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
