// plp_pair_dist.hpp -- closest points and Euclidean distances of listed CELL PAIRS of a packed table,
//     min |x - y|_2   s.t.  A_i x <= b_i,  A_j y <= b_j      for pair t = (i, j),
// pair_dist_kernel<D, RV> (plp_pair_dist.hip) behind plp_pair_dist.
//
// Method: GJK (Gilbert, Johnson, Keerthi 1988) on the Minkowski difference  M = P_i - P_j, whose point nearest to the origin
// is x - y.  The state is a simplex of at most D + 1 points w_k = p_k - q_k of M (p_k a support point of cell i, q_k of cell
// j) with barycentric weights lam.  One round, with v = x - y the current difference (before the first: xc_i - xc_j, e_0
// where that is zero) and u = v / |v|:
//   1  two support LPs through support::solve_one (plp_support.hpp, the lane walk on rows staged as a_i, beta_i = b_i -
//      a_i.xc):  p = argmax (-u).x over cell i,  q = argmax u.y over cell j;  lb = -h_i(-u) - h_j(u) = u.(p - q).
//      Every z of M has u.z >= lb, so dist* >= lb: weak duality.
//   2  stop when  dist - max(lb, 0) <= GAP_TOL E   (dist = |x - y|, E = max(1, |x|_inf, |y|_inf); not before a first simplex).
//   3  otherwise w = p - q joins the simplex with weight 0 and Wolfe's sub-algorithm (Math. Programming 11, 1976) finds
//      the point of conv{w_k} nearest to the origin: the affine minimiser alpha of the corral (Gram-Schmidt on the
//      differences w_k - w_0, nearest::gs_factor / ls_mult, every index a compile-time one); all alpha_k > 0: lam = alpha;
//      else lam moves towards alpha until a weight reaches zero, the points of weight zero leave (the slots above move down
//      by predicated moves: no array is indexed by a run-time number), again.  At most D + 1 such steps.
//   4  x = sum lam_k p_k,  y = sum lam_k q_k,  dist = |x - y|;  dist <= GAP_TOL E: the cells meet (to that tolerance), lb = 0.
// HANDED BACK (status 1): a support LP handed back (which covers a centre that is not strictly inside or not finite and rows
// that are not finite), the round cap, a corral that is affinely dependent to working precision (a weight that is not a
// number), a full simplex of D + 1 points that does not hold the origin to tolerance, and a STALL: the new point is one
// the simplex holds already, or dist did not fall, while the gap test fails.
//
// Before status 0 the final x is held against EVERY staged row of cell i and y against every row of cell j, recomputed
// from scratch:   (a_r.(x - xc) - beta_r) <= END_TOL E |a_r|   -- the feasibility rule of plp_nearest.hpp on unit-scaled slack.
//
// What a status 0 guarantees.  Let E as above, E_s >= E the largest extent max(1, |p|_inf, |h|) of the two support LPs of the
// last round.  x and y are convex combinations of support points, and by the end check lie within END_TOL E of every row's
// half-space, so   dist >= dist*_delta,  the distance of the cells with every row relaxed by delta = 1e-10 E |a_r|
// (for cells of inradius rho the exact dist* exceeds it by at most 2 delta R / rho, R their radius; as in plp_nearest.hpp the
// claim is the slab's).  For the other side, weak duality with the EXACT support values h*:
//     dist* >= L* = -h*_i(-u) - h*_j(u),   and per LP  h >= h* - 2e-10 E_s  (header of plp_support.hpp: the certificate's gap,
//     1e-10, and its residual term, below 1e-10 for optima within 100 max(1, |x'|) of the point), so
//     lb - L* = (h*_i - h_i) + (h*_j - h_j) <= 4e-10 E_s      (a support value that is too SMALL makes lb too large; one that
//                                                              is too large, h <= h* + 1e-10 E_s, only loosens lb)
//     dist - dist* <= (dist - max(lb, 0)) + (lb - L*) <= 1e-10 E + 4e-10 E_s.
// Together with the feasibility slack of the two points (2 * 1e-10 E on the other side):
//     -2e-10 E <= dist - dist* <= 5e-10 E_s,        c = 5 above, 2 below -- under the 1e-9 E the tests hold it to.
// For cells that meet, dist is the computed |x - y| <= 1e-10 E (exactly 0 where the simplex step returns the origin) and lb = 0.
//
// Raw status per pair:
//     0    settled, with the checks above
//     1    not settled here: dist = lb = x = y = NaN
//     3    a support LP came back unbounded (a cell is unbounded in a direction the iteration asked for; m = 0 is): NaN
//     255  PAIR_BAD: an index outside [0, n) or i = j (kernel only; nothing of the table is read for it)
// (a pair with one LP handed back and the other unbounded is 1.)
//
// The round cap.  MAX_ROUNDS = 16: the smallest value that cuts no pair of the test families which settles under a cap of 64.
// Measured on the host build over the tables of tests/test_pair_dist_host.py (seven soak families x six shapes, 200 listed
// pairs each, and every pair of the box grids of d = 1 .. 4): the settled pairs need at most
//     d = 1: 2,   d = 2: 6,   d = 3: 12,   d = 4: 16     support rounds (the stopping one included),
// and no pair ran into the cap of 64 (what was handed back there came from a support LP or a stall, after 1 .. 13 rounds).
// A pair the cap cuts is handed back like any other (DESIGN.md 4.23 has the table).
//
// The per-pair function compiles for the host as well (g++, tests/cabi/pair_dist_host.cpp): the same source, explicit fma
// and -ffp-contract=off on both sides.  NS is the number of sides a caller holds: 2 on the host (one call works both
// cells), 1 on the device (two lanes per pair, each walks one cell and keeps its own support points; both run the simplex
// step on the same w_k and get the same bits).  LP / BOTH are what differs: how the two LPs of a round are run and their
// answers brought together.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "plp_nearest.hpp"

namespace plp {
namespace pairdist {

constexpr int MAX_DIM = 4;
constexpr int PAIR_BAD = 255;
constexpr double GAP_TOL = 1e-10;                 // dist - max(lb, 0), and dist itself, relative to E
constexpr double END_TOL = support::END_TOL;      // feasibility of x and y on unit-scaled slack, relative to E
constexpr int MAX_ROUNDS = 16;

template <int D>
PLP_LANE_FN double dotd(const double (&a)[D], const double (&b)[D]) {
    return nearest::dotd<D>(a, b);
}

// The simplex: w_k and, per side held, the support points they came from; slots k >= n are zero.
template <int D, int NS>
struct Simplex {
    double w[D + 1][D], p[NS][D + 1][D], lam[D + 1];
    int n;
};

template <int D, int NS>
PLP_LANE_FN void clear(Simplex<D, NS>& S) {
    S.n = 0;
#pragma unroll
    for (int k = 0; k <= D; ++k) {
        S.lam[k] = 0.0;
#pragma unroll
        for (int c = 0; c < D; ++c) {
            S.w[k][c] = 0.0;
#pragma unroll
            for (int s = 0; s < NS; ++s) S.p[s][k][c] = 0.0;
        }
    }
}

// slot k leaves: the slots above it move down one place (predicated moves)
template <int D, int NS>
PLP_LANE_FN void drop(Simplex<D, NS>& S, const int k, const bool on) {
#pragma unroll
    for (int j = 0; j < D; ++j) {
        const bool mv = on & (j >= k);
        S.lam[j] = mv ? S.lam[j + 1] : S.lam[j];
#pragma unroll
        for (int c = 0; c < D; ++c) {
            S.w[j][c] = mv ? S.w[j + 1][c] : S.w[j][c];
#pragma unroll
            for (int s = 0; s < NS; ++s) S.p[s][j][c] = mv ? S.p[s][j + 1][c] : S.p[s][j][c];
        }
    }
    S.lam[D] = on ? 0.0 : S.lam[D];
#pragma unroll
    for (int c = 0; c < D; ++c) {
        S.w[D][c] = on ? 0.0 : S.w[D][c];
#pragma unroll
        for (int s = 0; s < NS; ++s) S.p[s][D][c] = on ? 0.0 : S.p[s][D][c];
    }
    S.n -= on ? 1 : 0;
}

// Wolfe's sub-algorithm on the n <= D + 1 points of S (the last one new, weight 0): on return lam >= 0 sums to 1 on an
// affinely independent corral, sum lam_k w_k the point of conv{w_k} nearest to the origin.  false: a number that is not
// finite (a dependent corral), or no end within D + 2 steps.
template <int D, int NS>
PLP_LANE_FN bool nearest_in_hull(Simplex<D, NS>& S, const bool go) {
    bool done = !go, ok = true;
#pragma unroll 1
    for (int it = 0; it < D + 2; ++it) {
        if (done) break;
        // the affine minimiser of the corral: w_0 + sum a_k (w_{k+1} - w_0),  a = argmin | -w_0 - sum a_k e_k |
        double e[D][D], t[D], a[D], al[D + 1];
#pragma unroll
        for (int k = 0; k < D; ++k) {
#pragma unroll
            for (int c = 0; c < D; ++c) e[k][c] = k + 1 < S.n ? S.w[k + 1][c] - S.w[0][c] : 0.0;
        }
#pragma unroll
        for (int c = 0; c < D; ++c) t[c] = -S.w[0][c];
        nearest::Gs<D> F;
        nearest::gs_factor<D>(e, S.n - 1, F);
        nearest::ls_mult<D>(F, t, a);
        double s = 0.0;
        bool fin = true, pos = true;
#pragma unroll
        for (int k = 0; k < D; ++k) {
            a[k] = k + 1 < S.n ? a[k] : 0.0;
            fin = fin & (a[k] - a[k] == 0.0);
            s += a[k];
            al[k + 1] = a[k];
        }
        al[0] = 1.0 - s;
        if (!fin) { ok = false; break; }
#pragma unroll
        for (int k = 0; k <= D; ++k) pos = pos & ((k >= S.n) | (al[k] > 0.0));
        if (pos) {
#pragma unroll
            for (int k = 0; k <= D; ++k) S.lam[k] = k < S.n ? al[k] : 0.0;
            done = true;
            break;
        }
        // towards alpha until the first weight reaches zero (lowest slot on ties)
        double th = 1.0;
        int kz = -1;
#pragma unroll
        for (int k = 0; k <= D; ++k) {
            const double den = S.lam[k] - al[k];
            const double r = den > 0.0 ? S.lam[k] / den : 0.0;
            const bool take = (k < S.n) & !(al[k] > 0.0) & ((kz < 0) | (r < th));
            th = take ? r : th;
            kz = take ? k : kz;
        }
#pragma unroll
        for (int k = 0; k <= D; ++k) {
            const double l = fma(th, al[k] - S.lam[k], S.lam[k]);
            S.lam[k] = ((k < S.n) & (k != kz) & (l > 0.0)) ? l : 0.0;
        }
#pragma unroll
        for (int k = D; k >= 0; --k) drop<D, NS>(S, k, (k < S.n) & !(S.lam[k] > 0.0));
        if (S.n < 1) { ok = false; break; }
    }
    return ok & done;
}

// x - xc against the staged rows of one cell: every (a_r.x' - beta_r) <= tol |a_r|  (a NaN fails)
template <int D, int RV>
PLP_LANE_FN bool inside_rows(const double* pA, const double* pbeta, const int LS, const double (&x)[D], const double (&xc)[4],
                             const double tol) {
    double xp[D];
#pragma unroll
    for (int k = 0; k < D; ++k) xp[k] = x[k] - xc[k];
    bool feas = true;
#pragma unroll 4
    for (int i = 0; i < RV; ++i) {
        double a[D];
        const double* base = pA + (size_t)(i * D) * LS;
#pragma unroll
        for (int k = 0; k < D; ++k) a[k] = base[k * LS];
        const double v = dotd<D>(a, xp) - pbeta[i * LS];
        feas = feas & (v <= tol * sqrt(dotd<D>(a, a)));
    }
    return feas;
}

// The iteration of one pair.  v0: the first direction (xc_i - xc_j).  go = false: no pair here (the caller still takes part
// in every round's LPs).  ANY(pred): true while any lane of the wavefront still runs (host: the predicate itself).
//   LP(run, u, pn, wn, lb, st): the two support LPs of a round in direction u (run = false: none wanted, but every lane
//       calls it) -> pn[NS][4] the new support point of each side held, wn = p - q, lb = -h_i(-u) - h_j(u), st = 0, or 1 / 3
//       as above.
//   BOTH(xs, xi, xj, f): from the points of the sides held, xs[NS][D], the points of both sides; f: (in) the sides held are
//       inside their rows to tol -- FEAS(xs, tol) -- (out) both are.
// -> dist, lb, xs (the closest points of the sides held), status, rounds (support rounds run for this pair).
template <int D, int NS, class AnyF, class LpF, class BothF, class FeasF>
PLP_LANE_FN void iterate(const double (&v0)[4], const bool go, AnyF ANY, LpF LP, BothF BOTH, FeasF FEAS, double& dist, double& lb,
                         double (&xs)[NS][D], int& status, int& rounds) {
    static_assert(D >= 1 && D <= MAX_DIM, "the simplex is held in registers for D <= 4");
    Simplex<D, NS> S;
    clear<D, NS>(S);
    double v[D], dd = __builtin_inf(), E = 1.0, lbv = 0.0;
    double vv = 0.0;
#pragma unroll
    for (int k = 0; k < D; ++k) {
        v[k] = v0[k];
        vv = fma(v[k], v[k], vv);
    }
    if (!(vv > 0.0)) {   // (a centre that is not a number: the LPs hand the pair back)
#pragma unroll
        for (int k = 0; k < D; ++k) v[k] = k == 0 ? 1.0 : 0.0;
    }
#pragma unroll
    for (int s = 0; s < NS; ++s) {
#pragma unroll
        for (int k = 0; k < D; ++k) xs[s][k] = 0.0;
    }
    enum : int { RUN = -1 };
    int st = go ? RUN : 1, rd = 0;
    bool conv = false;
#pragma unroll 1
    for (int round = 0; round < MAX_ROUNDS; ++round) {
        if (!ANY(st == RUN)) break;
        const bool run = st == RUN;
        const double vn = sqrt(dotd<D>(v, v));
        double u[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int k = 0; k < D; ++k) u[k] = run ? v[k] / vn : (k == 0 ? 1.0 : 0.0);
        double pn[NS][4], wn[4], l;
        int lst;
        LP(run, u, pn, wn, l, lst);
        if (!run) continue;
        ++rd;
        if (lst != 0) { st = lst; continue; }
        lbv = l;
        if (S.n > 0 && dd - fmax(lbv, 0.0) <= GAP_TOL * E) { conv = true; st = 0; continue; }
        // a point the simplex holds already, or a full simplex: nothing to add
        bool held = false;
#pragma unroll
        for (int k = 0; k <= D; ++k) {
            bool eq = k < S.n;
#pragma unroll
            for (int c = 0; c < D; ++c) eq = eq & (S.w[k][c] == wn[c]);
            held = held | eq;
        }
        if (held | (S.n > D)) { st = 1; continue; }
#pragma unroll
        for (int k = 0; k <= D; ++k) {
            const bool at = k == S.n;
#pragma unroll
            for (int c = 0; c < D; ++c) {
                S.w[k][c] = at ? wn[c] : S.w[k][c];
#pragma unroll
                for (int s = 0; s < NS; ++s) S.p[s][k][c] = at ? pn[s][c] : S.p[s][k][c];
            }
            S.lam[k] = at ? 0.0 : S.lam[k];
        }
        ++S.n;
        if (!nearest_in_hull<D, NS>(S, true)) { st = 1; continue; }
#pragma unroll
        for (int s = 0; s < NS; ++s) {
#pragma unroll
            for (int c = 0; c < D; ++c) {
                double a = S.lam[0] * S.p[s][0][c];
#pragma unroll
                for (int k = 1; k <= D; ++k) a = fma(S.lam[k], S.p[s][k][c], a);
                xs[s][c] = a;
            }
        }
        double xi[D], xj[D];
        bool f = true;
        BOTH(xs, xi, xj, f);
        double En = 1.0;
#pragma unroll
        for (int k = 0; k < D; ++k) {
            v[k] = xi[k] - xj[k];
            En = fmax(En, fmax(fabs(xi[k]), fabs(xj[k])));
        }
        const double dn = sqrt(dotd<D>(v, v));
        if (!(dn - dn == 0.0)) { st = 1; continue; }
        const bool fell = dn < dd;
        dd = dn;
        E = En;
        if (dd <= GAP_TOL * E) { conv = true; lbv = 0.0; st = 0; continue; }
        if (!fell) { st = 1; continue; }                // a stall
        if (S.n > D) { st = 1; continue; }              // D + 1 points that do not hold the origin to tolerance
    }
    if (st == RUN) st = 1;   // the cap
    // the end check: both points against every row of their cells (every lane of a pair goes through BOTH together)
    {
        double xi[D], xj[D];
        bool f = FEAS(xs, END_TOL * E);
        BOTH(xs, xi, xj, f);
        if (st == 0 && !(conv & f)) st = 1;
    }
    const double qnan = __builtin_nan("");
    status = st;
    rounds = rd;
    dist = st == 0 ? dd : qnan;
    lb = st == 0 ? fmin(fmax(lbv, 0.0), dd) : qnan;   // (rounding may put u.(p - q) an ulp above |x - y|: dist bounds dist* too)
#pragma unroll
    for (int s = 0; s < NS; ++s) {
#pragma unroll
        for (int k = 0; k < D; ++k) xs[s][k] = st == 0 ? xs[s][k] : qnan;
    }
}

// One support LP of a round for one side: cell rows pA / pbeta (plp_support.hpp's layout), sgn = -1 for cell i (direction
// -u), +1 for cell j -> h, the point, solve_one's status.
template <int D, int RV, class AnyF>
PLP_LANE_FN void side_lp(const double* pA, const double* pbeta, const int LS, const int m, const double (&xc)[4], const double sgn,
                         const double (&u)[4], const bool run, AnyF ANY, double& h, double (&x)[4], int& st) {
    double c[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int k = 0; k < D; ++k) c[k] = sgn * u[k];
    support::solve_one<D, RV>(pA, pbeta, LS, m, c, xc, run, ANY, h, x, st);
}

// the two LP statuses of a round as one: 0, or 1 where either was handed back, else 3
PLP_LANE_FN int lp_status(const int si, const int sj) {
    return ((si == 0) & (sj == 0)) ? 0 : (((si == 1) | (sj == 1)) ? 1 : (((si == 3) | (sj == 3)) ? 3 : 1));
}

// Both cells in one call (the host build; NS = 2).  Rows of cell i at pAi / pbi, of cell j at pAj / pbj (LS apart).
template <int D, int RV>
PLP_LANE_FN void solve_pair(const double* pAi, const double* pbi, const int mi, const double (&xci)[4], const double* pAj,
                            const double* pbj, const int mj, const double (&xcj)[4], const int LS, double& dist, double& lb,
                            double (&x)[D], double (&y)[D], int& status, int& rounds) {
    auto any = [](bool q) { return q; };
    double v0[4] = {0.0, 0.0, 0.0, 0.0}, xs[2][D];
#pragma unroll
    for (int k = 0; k < D; ++k) v0[k] = xci[k] - xcj[k];
    iterate<D, 2>(
        v0, true, any,
        [&](const bool run, const double(&u)[4], double(&pn)[2][4], double(&wn)[4], double& l, int& st) {
            double hi, hj;
            int si, sj;
            side_lp<D, RV>(pAi, pbi, LS, mi, xci, -1.0, u, run, any, hi, pn[0], si);
            side_lp<D, RV>(pAj, pbj, LS, mj, xcj, 1.0, u, run, any, hj, pn[1], sj);
#pragma unroll
            for (int k = 0; k < 4; ++k) wn[k] = pn[0][k] - pn[1][k];
            l = -hi - hj;
            st = lp_status(si, sj);
        },
        [&](const double(&p)[2][D], double(&xi)[D], double(&xj)[D], bool&) {
#pragma unroll
            for (int k = 0; k < D; ++k) {
                xi[k] = p[0][k];
                xj[k] = p[1][k];
            }
        },
        [&](const double(&p)[2][D], const double tol) {
            return inside_rows<D, RV>(pAi, pbi, LS, p[0], xci, tol) & inside_rows<D, RV>(pAj, pbj, LS, p[1], xcj, tol);
        },
        dist, lb, xs, status, rounds);
#pragma unroll
    for (int k = 0; k < D; ++k) {
        x[k] = xs[0][k];
        y[k] = xs[1][k];
    }
}

}  // namespace pairdist
}  // namespace plp
