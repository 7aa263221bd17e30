// plp_reduce_rules.hpp -- the rules of the reference's reduce() (polytope/polytope.py:1053-1163) and bounding box (:1314-1411),
// each stated ONCE for reduce_general_tile, reduce_r_tile / reduce_wsplit_kernel / f2_presolve(_ws), reduce_lane_tile,
// reduce_lds_kernel and the stand-alone box kernels.  A rule is the arithmetic and comparison the reference dictates:
// scalars by value, at most two results by reference.  Who owns a row, which ballot gathers what, the loop around a rule and
// a term only one kernel has stay at the kernel.  The independent restatement the tests compare against: plpo_reduce /
// bbox_impl in oracle/plp_oracle.c (the presolve has no twin there: the oracle solves every LP).
#pragma once
#include "plp_common.hpp"

namespace plp { namespace rule {

constexpr double qnan = __builtin_bit_cast(double, 0x7ff8000000000000ll);
constexpr double pinf = __builtin_bit_cast(double, 0x7ff0000000000000ll);
constexpr double PREFILTER_MARGIN = 1e-4;   // a row leaves when the box puts it this far inside (:1134)
constexpr double RHS_SHIFT = 0.1;           // h[k] += 0.1 for row k's redundancy LP, -= 0.1 after it (:1149-1151)
constexpr double BBOX_MIN_R = 1e-6;         // (the engines' own) smallest Chebyshev radius the stand-alone boxes start from
constexpr double PRESOLVE_REL = 1e-9;       // tau = abs_tol + PRESOLVE_REL (1 + |b_k| + s_k)
constexpr double PRESOLVE_TAU_MAX = 0.05;   // tau stays well inside the relaxed row k (RHS_SHIFT)
constexpr double PRESOLVE_T1_BACKOFF = 1.0 - 0x1p-40;   // the first leg stops a hair before the blocking row
constexpr double PRESOLVE_MIN_SIN2 = 1e-12; // a_k.d > this |a_k|^2: rows k and j are not parallel
constexpr double PRESOLVE_T2_MAX = 1e300;   // a finite second leg

// ---- F1 verdicts (cheby_ball :1289-1297, is_fulldim :1081); f1_open: neither optimal nor infeasible (RF_F1OPEN)
__device__ __forceinline__ bool ball_ok(int st, double r) { return (st == ST_OPT) & (r >= 0.0); }
__device__ __forceinline__ bool full_dim(bool ball, double r, double abs_tol) { return ball & (r > abs_tol); }
__device__ __forceinline__ bool f1_open(int st) { return (st != ST_OPT) & (st != ST_INFEAS); }
__device__ __forceinline__ int empty_flags(bool f1open) { return RF_EMPTY | (f1open ? RF_F1OPEN : 0); }

// ---- dedupe (:1094-1110) on unit rows: of a pair of the same plane the larger normalised offset goes, ties drop the lower index.
// row_goes and pair_loser are the SAME rule, row_goes(i, j, b_i, b_j) == (pair_loser(lo, hi, b_lo, b_hi) == i); both stay because
// the sites differ in what they hold: a lane that walks row i's partners, or one evaluation that settles both rows of a pair.
__device__ __forceinline__ bool same_plane(double dot, double abs_tol) { return dot > 1.0 - abs_tol; }
__device__ __forceinline__ bool row_goes(int i, int j, double bi, double bj) { return (i < j) ? !(bi < bj) : (bj < bi); }
__device__ __forceinline__ int pair_loser(int lo, int hi, double blo, double bhi) { return (blo < bhi) ? hi : lo; }

// ---- stage rule: early return after the dedupe and after the box (:1114-1116, :1136-1138), else the box first (:1118)
__device__ __forceinline__ bool few_rows(int neq, int d) { return neq <= d + 1; }
__device__ __forceinline__ bool box_first(int neq, int d) { return neq > 3 * d; }

// ---- box LP read-out (:1367-1409).  From the centre: zeta = c.x' = -negz, x_k = xc_k + x'_k, lower: c = +e_k, upper: c = -e_k.
// box_value: unbounded -> -+inf (:1376, :1398), any other status -> NaN and `fail` (:1378-1384); `opt`: the optimum's coordinate.
__device__ __forceinline__ double box_optimum(bool up, double xck, double negz) { return up ? (xck + negz) : (xck - negz); }
__device__ __forceinline__ double box_value(int st, bool up, double opt, bool& fail) {
    fail = (st != ST_OPT) & (st != ST_UNBND);
    return st == ST_OPT ? opt : (st == ST_UNBND ? (up ? pinf : -pinf) : qnan);
}

// ---- prefilter (:1131-1134): the sums of one row, coordinate by coordinate in k order, and the cut
__device__ __forceinline__ void prefilter_add(double aik, double lo, double hi, double& s1, double& s2) {
    const double pa = (aik > 0.0 ? 1.0 : 0.0) * aik;
    s1 = s1 + pa * (hi - lo);
    s2 = s2 + aik * lo;
}
__device__ __forceinline__ bool prefilter_drops(double s1, double s2, double b) { return (s1 - (b - s2)) < -PREFILTER_MARGIN; }

// ---- F2 (:1142-1160), h[k] shifted in place.  f2_rhs: a row's h in LP k (`before`: it had its LP, the round trip stays; `own`: k)
__device__ __forceinline__ double rhs_relaxed(double b) { return b + RHS_SHIFT; }        // (:1149)
__device__ __forceinline__ double rhs_restored(double bup) { return bup - RHS_SHIFT; }   // (:1151), of a relaxed value
__device__ __forceinline__ double rhs_round_trip(double b) { return rhs_restored(rhs_relaxed(b)); }
__device__ __forceinline__ double f2_rhs(bool before, bool own, double b) {
    return before ? rhs_round_trip(b) : (own ? rhs_relaxed(b) : b);
}
__device__ __forceinline__ double f2_objective(double fun, double hk) { return -fun - hk; }   // (:1156), hk after its round trip
__device__ __forceinline__ bool f2_keeps(int st, double obj, double tol) { return ((st == ST_OPT) & (obj > tol)) | (st == ST_UNBND); }

// ---- ray presolve of F2 (derivation: f2_presolve, plp_reduce_r_impl.hpp).  Candidate k: slack s_k, g_kk = |a_k|^2, skt = s_k +
// tau.  NaN-safe: a row that fails a comparison is never settled.  presolve_clear: row i does not stop the ray along a_k.
// presolve_second: the witness past the blocking row j (a_j.a_k > 0, t1 |a_k|^2 < s_k + tau; anything else goes to the simplex).
__device__ __forceinline__ bool presolve_reach(double bk, double sk, double abs_tol, double gkk, double& skt) {
    const double tau = abs_tol + PRESOLVE_REL * (1.0 + fabs(bk) + sk);
    skt = sk + tau;
    return (gkk > 0.0) & (tau < PRESOLVE_TAU_MAX);
}
__device__ __forceinline__ bool presolve_clear(double skt, double gik, double si, double gkk) { return skt * gik <= si * gkk; }
__device__ __forceinline__ bool presolve_second(double sj, double gjk, double gjj, double gkk, double skt, double& c1, double& c2) {
    const double rho = gjk / gjj;
    const double t1 = (sj / gjk) * PRESOLVE_T1_BACKOFF;
    const double akd = fma(-rho, gjk, gkk);       // a_k.d = |a_k|^2 - (a_j.a_k)^2 / |a_j|^2 >= 0
    const double t2 = fma(-t1, gkk, skt) / akd;   // (s_k + tau - t1 |a_k|^2) / a_k.d
    c1 = t1 + t2;
    c2 = t2 * rho;
    return (gjk > 0.0) & (akd > PRESOLVE_MIN_SIN2 * gkk) & (t2 >= 0.0) & (t2 < PRESOLVE_T2_MAX);
}
__device__ __forceinline__ bool presolve_clear2(double c1, double c2, double gik, double gij, double si) {
    return fma(-c2, gij, c1 * gik) <= si;
}

} }  // namespace plp::rule
