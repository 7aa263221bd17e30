// plp_nearest.hpp -- nearest points and Euclidean distances to polytopes,  min 1/2 |x - p|^2  s.t.  A x <= b,  for MANY points
// per polytope, the rows read once: nearest_kernel<D, RV> (plp_nearest.hip) behind plp_nearest_batch.
//
// Not an LP: a strictly convex QP with the identity as Hessian, solved per lane by a dual active-set walk in the manner of
// Goldfarb and Idnani (Math. Programming 27, 1983).  The tiles, the LDS layout and the frame of the kernel are those of
// plp_row_tile.hpp, with two staged scalars per row (beta_i, |a_i|); plp_support.hpp gives the three end tolerances.
//
// Rows.  Staged at unit 2-norm,  n_i = a_i / |a_i|,  beta_i = b_i / |a_i|,  with |a_i| kept beside them (the multipliers are
// given back with respect to the rows as passed).  A zero row with b_i >= 0 binds nowhere and is staged as (0, 0); a zero row
// with b_i < 0 is staged as (0, -1): it is violated everywhere and is its own Farkas certificate (extreme_batch's rule).
// Rows i >= m are (0, 0).  A row that is not finite is staged as NaN and every problem of that polytope comes back as 1.
//
// The walk.  x = p, W = {} (the active set, at most D rows, in registers), u = () (its multipliers):  x = p - sum u_j n_j
// holds throughout.  Repeat:
//   1  t = the most violated row, the largest n_i.x - beta_i (lowest index on ties); none above STOP_TOL E: the end.
//   2  r = argmin | n_t - sum_j r_j n_j |  over W  (Gram-Schmidt on the rows of W: the Cholesky factor of their Gram matrix,
//      at most 4 x 4, every index a compile-time one),  z = -(n_t - sum r_j n_j): the step that lowers n_t.x with W held.
//      |z|^2 <= DEP_TOL (n_t in the span of W to working precision, always so at |W| = D): no step in x, tau2 = inf; else
//      tau2 = (n_t.x - beta_t) / |z|^2, the length that reaches row t.
//      tau1 = min { u_j / r_j : r_j > 0 }: the length at which a multiplier of W would turn negative, k its row.
//   3  tau1 = tau2 = inf:  n_t = sum r_j n_j with r <= 0 while every row of W is tight and t violated -- the polytope is
//      EMPTY, y = (1, -r) the Farkas combination on |W| + 1 <= D + 1 rows.
//      tau1 < tau2:  a partial step -- x += tau1 z, u -= tau1 r, u_t += tau1, row k leaves W, back to 2 with the same t.
//      otherwise  :  the full step -- x += tau2 z, u -= tau2 r, t joins W with u_t + tau2, back to 1.
// Every step with tau > 0 raises the dual objective, so no active set returns; what is left to chance (steps of length
// zero at a degenerate point) is counted.  The walk HANDS BACK (status 1) when it is not sure: ZERO_RUN steps of length zero
// in a row, the most violated row already in W (rows a hair apart), a number that is not finite, or the cap
//     iter_cap(m, D) = 2 (m + 2 D) + 4     steps, partial and full together
// (each row joins W twice and every join is paid for with at most two leaves; the soak's longest walk is far below it).
// Before the end checks the rows of W are made tight once more (x -= N^T G^-1 (N x - beta): a correction in the span of W,
// so x = p - N^T u stays true); a point that violates no row never enters any of this and comes back as p, bit for bit.
//
// End checks, in plain doubles on the final point against EVERY staged row, recomputed from scratch (nothing of the walk's
// u, nor of its bookkeeping, is used):  E = max(1, |x|_inf, |p|_inf),
//     feasibility   max_i (n_i.x - beta_i) <= END_TOL E
//     optimality    lam = least-squares multipliers of p - x on the rows of W (ls_mult below, mirroring support::ls_multipliers),
//                   one round of refinement, negative entries set to 0;
//                   gap = sum lam_j |beta_j - n_j.x| <= OPT_TOL_GAP E max(|x - p|, OPT_TOL_GAP E)
//                   r = (p - x) - sum lam_j n_j,  |r|_2 <= OPT_TOL_RES E.
// What that proves (f(y) = 1/2 |y - p|^2, x* the nearest point, x feasible, lam >= 0 ANY numbers):
//     f(y) - f(x) = (x - p).(y - x) + 1/2 |y - x|^2                                   (f is quadratic with Hessian I)
//     (x - p).(y - x) = -sum lam_j n_j.(y - x) - r.(y - x)
//                     >= -sum lam_j (beta_j - n_j.x) - |r| |y - x|  >=  -gap - |r| |y - x|      for every feasible y,
// and f(x*) <= f(x), so with s = |x* - x|:   0 >= -gap - |r| s + s^2 / 2,  i.e.
//     |x - x*| <= |r| + sqrt(|r|^2 + 2 gap),
//     dist - dist* = 2 (f(x) - f(x*)) / (dist + dist*) <= 2 (gap + |r| s) / (dist + dist*) <= 2 (gap + |r| s) / dist.
// Unlike the LP certificate of plp_support.hpp this is a BOUND: strict convexity leaves no optimal face to reach along.
// With the constants: gap <= 1e-10 E dist gives dist - dist* <= 2e-10 E + 2e-12 E s / dist, and for dist below 1e-10 E the
// floor gap <= 1e-20 E^2 gives s <= 1.5e-10 E.  (x may be OUTSIDE a row by END_TOL E: then dist >= dist* - 1e-10 E is not
// implied by the above but by x lying within 1e-10 E of the slab -- the tests hold dist to 1e-9 E on both sides.)
// The constants are those of plp_support.hpp (END_TOL, OPT_TOL_GAP, OPT_TOL_RES): the derivation asks for no other; what
// changes is their meaning -- the gap is held against E times the DISTANCE, because it enters dist through gap / dist.
//
// Status 2 (empty) is given only when the Farkas combination passes its own check here:
//     y >= 0,   | sum y_j n_j |_1 <= FARKAS_RES sum y_j,   sum y_j beta_j < -FARKAS_GAP sum y_j
// (any x has  sum y_j (n_j.x - beta_j) >= -|sum y_j n_j|_1 |x|_inf - sum y_j beta_j > 0  while |x|_inf < 100: some row is
// violated at every such x; beyond that extent the claim rests on the residual being rounding).  Otherwise: handed back.
//
// Raw status per (polytope, point):
//     0  optimum, both end checks passed
//     2  the polytope is empty (certified as above): dist = x = NaN
//     1  not settled here: dist = x = NaN, face = 0, lam = 0
//
// The per-problem function compiles for the host as well (g++, tests/cabi/nearest_host.cpp): the same source, explicit fma
// and -ffp-contract=off on both sides.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "plp_support.hpp"

namespace plp {
namespace nearest {

constexpr int MAX_DIM = 4;
constexpr double END_TOL = support::END_TOL;            // feasibility, relative to E
constexpr double OPT_TOL_GAP = support::OPT_TOL_GAP;    // complementary slackness, relative to E max(dist, OPT_TOL_GAP E)
constexpr double OPT_TOL_RES = support::OPT_TOL_RES;    // |(p - x) - sum lam_j n_j|_2, relative to E
constexpr double FARKAS_RES = 1e-12, FARKAS_GAP = 1e-10;
constexpr double STOP_TOL = 1e-12;   // the walk stops when no row is violated by more than this times E (END_TOL / 100)
constexpr double DEP_TOL = 1e-12;    // |z|^2 below this: n_t is taken as dependent on W (an angle of 1e-6 to their span)
constexpr int ZERO_RUN = 6;          // steps of length zero in a row before the walk hands back
constexpr int K_ROUNDS = 8;          // rounds of one K-chunk (rowtile::chunk_rounds): rows are staged once per 8 rounds at most

constexpr int iter_cap(int m, int D) { return 2 * (m + 2 * D) + 4; }
using rowtile::polytopes_per_group, rowtile::row_slots;   // (as in plp_support.hpp)
// rounds of a K-chunk for L lanes per polytope
constexpr int chunk_rounds(int K, int L) { return rowtile::chunk_rounds(K, L, K_ROUNDS); }

template <int D>
PLP_LANE_FN double dotd(const double (&a)[D], const double (&b)[D]) {
    double s = a[0] * b[0];
#pragma unroll
    for (int k = 1; k < D; ++k) s = fma(a[k], b[k], s);
    return s;
}

// One row as the kernel stages it: a (D entries), bi -> n, beta, nrm
template <int D>
PLP_LANE_FN void stage_row(const double* a, const double bi, const bool live, double (&n)[D], double& beta, double& nrm) {
    double v[D];
#pragma unroll
    for (int k = 0; k < D; ++k) v[k] = live ? a[k] : 0.0;
    const double bb = live ? bi : 0.0;
    const double nn = sqrt(dotd<D>(v, v));
    const bool zero = nn == 0.0;                 // (a NaN is not zero: it goes through the division)
    const bool fin = (nn - nn == 0.0) & (bb - bb == 0.0);
    const double qnan = __builtin_nan("");
#pragma unroll
    for (int k = 0; k < D; ++k) n[k] = zero ? 0.0 : (fin ? v[k] / nn : qnan);
    beta = zero ? (bb >= 0.0 ? 0.0 : (bb < 0.0 ? -1.0 : qnan)) : (fin ? bb / nn : qnan);
    nrm = zero ? 1.0 : nn;
}

// Gram-Schmidt without square roots on the first `q` of D rows (the others are zero rows):  q_j = n_j - sum_{i<j} mu_ji q_i,
// qq_j = q_j.q_j (1 for j >= q).  Dependent rows give qq_j = 0 and numbers that are not: the end checks then fail.
template <int D>
struct Gs {
    double q[D][D], mu[D][D], qq[D];
};

template <int D>
PLP_LANE_FN void gs_factor(const double (&n)[D][D], const int nq, Gs<D>& F) {
#pragma unroll
    for (int j = 0; j < D; ++j) {
#pragma unroll
        for (int k = 0; k < D; ++k) F.q[j][k] = n[j][k];
#pragma unroll
        for (int i = 0; i < j; ++i) {
            F.mu[j][i] = dotd<D>(F.q[j], F.q[i]) / F.qq[i];
#pragma unroll
            for (int k = 0; k < D; ++k) F.q[j][k] = fma(-F.mu[j][i], F.q[i][k], F.q[j][k]);
        }
        const double s = dotd<D>(F.q[j], F.q[j]);
        F.qq[j] = j < nq ? s : 1.0;
    }
}

// lam = argmin | v - sum_j lam_j n_j |_2  (support::ls_multipliers for D columns)
template <int D>
PLP_LANE_FN void ls_mult(const Gs<D>& F, const double (&v)[D], double (&lam)[D]) {
    double g[D], r[D];
#pragma unroll
    for (int k = 0; k < D; ++k) r[k] = v[k];
#pragma unroll
    for (int j = 0; j < D; ++j) {
        g[j] = dotd<D>(r, F.q[j]) / F.qq[j];
#pragma unroll
        for (int k = 0; k < D; ++k) r[k] = fma(-g[j], F.q[j][k], r[k]);
    }
#pragma unroll
    for (int j = D - 1; j >= 0; --j) {
        double s = g[j];
#pragma unroll
        for (int i = j + 1; i < D; ++i) s = fma(-F.mu[i][j], lam[i], s);
        lam[j] = s;
    }
}

// dx in the span of the rows with  n_j.dx = -s_j  for j < q  (n_j = q_j + sum_{i<j} mu_ji q_i: forward substitution)
template <int D>
PLP_LANE_FN void tighten(const Gs<D>& F, const int nq, const double (&s)[D], double (&dx)[D]) {
    double a[D];
#pragma unroll
    for (int k = 0; k < D; ++k) dx[k] = 0.0;
#pragma unroll
    for (int j = 0; j < D; ++j) {
        double t = -s[j];
#pragma unroll
        for (int i = 0; i < j; ++i) t = fma(-F.mu[j][i] * F.qq[i], a[i], t);
        a[j] = j < nq ? t / F.qq[j] : 0.0;
#pragma unroll
        for (int k = 0; k < D; ++k) dx[k] = fma(a[j], F.q[j][k], dx[k]);
    }
}

// One point of one polytope.  pN / pbeta / pnrm: the polytope's staged rows -- n_i[k] at pN[(i * D + k) * LS], beta_i at
// pbeta[i * LS], |a_i| at pnrm[i * LS], RV row slots.  m: its rows (for the cap only; slots i >= m are zero rows).
// -> dist, x, face (bit i: row i in the final active set), lam (with respect to the rows as given, ascending row order,
// zero-padded), status.
template <int D, int RV>
PLP_LANE_FN void solve_one(const double* pN, const double* pbeta, const double* pnrm, const int LS, const int m,
                           const double (&p)[D], double& dist, double (&x)[D], uint64_t& face, double (&lam)[D], int& status) {
    static_assert(D >= 1 && D <= MAX_DIM, "the active set is held in registers for D <= 4");
    static_assert(RV <= rowtile::MAX_ROWS, "face is one 64-bit word");
    auto row_of = [&](const int i, double (&a)[D]) {
        const double* base = pN + (size_t)(i * D) * LS;
#pragma unroll
        for (int k = 0; k < D; ++k) a[k] = base[k * LS];
    };
    // the most violated row at y (lowest index on ties); fin: every n_i.y - beta_i is a finite number
    auto scan = [&](const double (&y)[D], double& vmax, int& imax, bool& fin) {
        vmax = -__builtin_inf();
        imax = -1;
        fin = true;
#pragma unroll 4
        for (int i = 0; i < RV; ++i) {
            double a[D];
            row_of(i, a);
            const double v = dotd<D>(a, y) - pbeta[i * LS];
            fin = fin & (v - v == 0.0);
            const bool up = v > vmax;
            vmax = up ? v : vmax;
            imax = up ? i : imax;
        }
    };
    double pinf = 0.0;
#pragma unroll
    for (int k = 0; k < D; ++k) {
        x[k] = p[k];
        pinf = fmax(pinf, fabs(p[k]));   // (fmax drops a NaN: the scan sees it)
    }
    double n[D][D], u[D], y[D + 1];
    int w[D], yi[D + 1];
#pragma unroll
    for (int j = 0; j < D; ++j) {
        u[j] = 0.0;
        w[j] = -1;
#pragma unroll
        for (int k = 0; k < D; ++k) n[j][k] = 0.0;
    }
#pragma unroll
    for (int j = 0; j <= D; ++j) {
        y[j] = 0.0;
        yi[j] = -1;
    }
    enum : int { RUN = -1, DONE = 0, HAND = 1, EMPTY = 2 };
    int nq = 0, t = -1, st = RUN, zero_run = 0;
    double nt[D], bt = 0.0, ut = 0.0;
#pragma unroll
    for (int k = 0; k < D; ++k) nt[k] = 0.0;
    const int cap = iter_cap(m, D);
    for (int it = 0; it < cap && st == RUN; ++it) {
        if (t < 0) {
            double vmax;
            int imax;
            bool fin;
            scan(x, vmax, imax, fin);
            double E = fmax(1.0, pinf);
#pragma unroll
            for (int k = 0; k < D; ++k) E = fmax(E, fabs(x[k]));
            if (!fin) { st = HAND; break; }
            if (!(vmax > STOP_TOL * E)) { st = DONE; break; }
            bool held = false;
#pragma unroll
            for (int j = 0; j < D; ++j) held = held | ((j < nq) & (w[j] == imax));
            if (held) { st = HAND; break; }
            t = imax;
            row_of(t, nt);
            bt = pbeta[t * LS];
            ut = 0.0;
        }
        Gs<D> F;
        gs_factor<D>(n, nq, F);
        double r[D], z[D];
        ls_mult<D>(F, nt, r);
#pragma unroll
        for (int k = 0; k < D; ++k) {
            double s = nt[k];
#pragma unroll
            for (int j = 0; j < D; ++j) s = fma(-r[j], n[j][k], s);
            z[k] = -s;
        }
        const double zz = dotd<D>(z, z);
        const bool dep = (nq == D) | !(zz > DEP_TOL);
        const double v = dotd<D>(nt, x) - bt;
        const double inf = __builtin_inf();
        const double tau2 = dep ? inf : v / zz;
        double tau1 = inf;
        int k1 = -1;
        bool num = !(zz - zz == 0.0);
#pragma unroll
        for (int j = 0; j < D; ++j) {
            num = num | ((j < nq) & !(r[j] - r[j] == 0.0));
            const double c = u[j] / r[j];
            const bool take = (j < nq) & (r[j] > 0.0) & (c < tau1);
            tau1 = take ? c : tau1;
            k1 = take ? j : k1;
        }
        if (num) { st = HAND; break; }
        if (k1 < 0 && dep) {   // n_t = sum r_j n_j, r <= 0: empty
            y[D] = 1.0;
            yi[D] = t;
#pragma unroll
            for (int j = 0; j < D; ++j) {
                y[j] = j < nq ? -r[j] : 0.0;
                yi[j] = j < nq ? w[j] : -1;
            }
            st = EMPTY;
            break;
        }
        const bool partial = tau1 < tau2;
        const double tau = partial ? tau1 : tau2;
        if (!dep) {
#pragma unroll
            for (int k = 0; k < D; ++k) x[k] = fma(tau, z[k], x[k]);
        }
#pragma unroll
        for (int j = 0; j < D; ++j) {
            const double uj = fma(-tau, r[j], u[j]);
            u[j] = j < nq ? (uj > 0.0 ? uj : 0.0) : 0.0;
        }
        ut += tau;
        if (partial) {
            // row k1 leaves: the rows above it move down one place
#pragma unroll
            for (int j = 0; j + 1 < D; ++j) {
                const bool mv = j >= k1;
                u[j] = mv ? u[j + 1] : u[j];
                w[j] = mv ? w[j + 1] : w[j];
#pragma unroll
                for (int k = 0; k < D; ++k) n[j][k] = mv ? n[j + 1][k] : n[j][k];
            }
            u[D - 1] = 0.0;
            w[D - 1] = -1;
#pragma unroll
            for (int k = 0; k < D; ++k) n[D - 1][k] = 0.0;
            --nq;
            zero_run = tau > 0.0 ? 0 : zero_run + 1;
            if (zero_run >= ZERO_RUN) st = HAND;
        } else {
#pragma unroll
            for (int j = 0; j < D; ++j) {
                const bool at = j == nq;
                u[j] = at ? ut : u[j];
                w[j] = at ? t : w[j];
#pragma unroll
                for (int k = 0; k < D; ++k) n[j][k] = at ? nt[k] : n[j][k];
            }
            ++nq;
            t = -1;
        }
    }
    if (st == RUN) st = HAND;   // the cap
    const double qnan = __builtin_nan("");
    face = 0;
#pragma unroll
    for (int j = 0; j < D; ++j) lam[j] = 0.0;
    if (st == EMPTY) {
        // the Farkas combination, checked: y >= 0, |sum y_j n_j|_1 <= FARKAS_RES sum y_j, sum y_j beta_j < -FARKAS_GAP sum y_j
        double sy = 0.0, sb = 0.0, sn[D];
        bool pos = true;
#pragma unroll
        for (int k = 0; k < D; ++k) sn[k] = 0.0;
#pragma unroll
        for (int j = 0; j <= D; ++j) {
            const bool on = yi[j] >= 0;
            const int i = on ? yi[j] : 0;
            double a[D];
            row_of(i, a);
            const double yj = on ? y[j] : 0.0;
            pos = pos & (yj >= 0.0);
            sy += yj;
            sb = fma(yj, pbeta[i * LS], sb);
#pragma unroll
            for (int k = 0; k < D; ++k) sn[k] = fma(yj, a[k], sn[k]);
        }
        double s1 = 0.0;
#pragma unroll
        for (int k = 0; k < D; ++k) s1 += fabs(sn[k]);
        status = (pos & (s1 <= FARKAS_RES * sy) & (sb < -FARKAS_GAP * sy)) ? 2 : 1;
    } else if (st == DONE) {
        double sl[D];
        if (nq > 0) {
            // the rows of W made tight once more
            Gs<D> F;
            gs_factor<D>(n, nq, F);
            double s[D], dx[D];
#pragma unroll
            for (int j = 0; j < D; ++j) s[j] = j < nq ? dotd<D>(n[j], x) - pbeta[(w[j] < 0 ? 0 : w[j]) * LS] : 0.0;
            tighten<D>(F, nq, s, dx);
#pragma unroll
            for (int k = 0; k < D; ++k) x[k] += dx[k];
        }
        // end check 1, feasibility: the final point against every staged row
        double vmax;
        int imax;
        bool fin;
        scan(x, vmax, imax, fin);
        double E = fmax(1.0, pinf), v[D];
#pragma unroll
        for (int k = 0; k < D; ++k) {
            E = fmax(E, fabs(x[k]));
            v[k] = p[k] - x[k];
        }
        const bool feas = fin & (vmax <= END_TOL * E);
        // end check 2, optimality: multipliers on the rows of W, from scratch
        bool opt = true;
        const double dd = sqrt(dotd<D>(v, v));
        double l[D];
#pragma unroll
        for (int j = 0; j < D; ++j) l[j] = 0.0;
        if (nq > 0) {
            Gs<D> F;
            gs_factor<D>(n, nq, F);
            double dl[D], r[D];
            ls_mult<D>(F, v, l);
#pragma unroll
            for (int k = 0; k < D; ++k) {
                double s = v[k];
#pragma unroll
                for (int j = 0; j < D; ++j) s = fma(-l[j], n[j][k], s);
                r[k] = s;
            }
            ls_mult<D>(F, r, dl);
            double gap = 0.0;
#pragma unroll
            for (int j = 0; j < D; ++j) {
                l[j] = l[j] + dl[j];
                l[j] = l[j] > 0.0 ? l[j] : (l[j] <= 0.0 ? 0.0 : l[j]);   // (a NaN stays)
                l[j] = j < nq ? l[j] : 0.0;
                sl[j] = j < nq ? pbeta[(w[j] < 0 ? 0 : w[j]) * LS] - dotd<D>(n[j], x) : 0.0;
                gap = fma(l[j], fabs(sl[j]), gap);
            }
            double r2 = 0.0;
#pragma unroll
            for (int k = 0; k < D; ++k) {
                double s = v[k];
#pragma unroll
                for (int j = 0; j < D; ++j) s = fma(-l[j], n[j][k], s);
                r2 = fma(s, s, r2);
            }
            opt = (gap <= OPT_TOL_GAP * E * fmax(dd, OPT_TOL_GAP * E)) & (sqrt(r2) <= OPT_TOL_RES * E);
        } else {
            opt = dd == 0.0;   // (no step was taken: x is p)
        }
        status = (feas & opt) ? 0 : 1;
        if (status == 0) {
            // the rows of W in ascending order (a compare-exchange network on at most four), lam with respect to a_i
            double lo[D];
            int wo[D];
#pragma unroll
            for (int j = 0; j < D; ++j) {
                const bool on = j < nq;
                wo[j] = on ? w[j] : 0x7fffffff;
                lo[j] = on ? l[j] / pnrm[(on ? w[j] : 0) * LS] : 0.0;
                face |= on ? (uint64_t)1 << (w[j] & 63) : (uint64_t)0;
            }
#pragma unroll
            for (int a = 0; a < D; ++a) {
#pragma unroll
                for (int j = 0; j + 1 < D - a; ++j) {
                    const bool sw = wo[j] > wo[j + 1];
                    const int wi = wo[j];
                    const double li = lo[j];
                    wo[j] = sw ? wo[j + 1] : wo[j];
                    lo[j] = sw ? lo[j + 1] : lo[j];
                    wo[j + 1] = sw ? wi : wo[j + 1];
                    lo[j + 1] = sw ? li : lo[j + 1];
                }
            }
#pragma unroll
            for (int j = 0; j < D; ++j) lam[j] = lo[j];
            dist = dd;
        }
    } else {
        status = 1;
    }
    if (status != 0) {
        dist = qnan;
        face = 0;
#pragma unroll
        for (int k = 0; k < D; ++k) {
            x[k] = qnan;
            lam[k] = 0.0;
        }
    }
}

}  // namespace nearest
}  // namespace plp
