// plp_projhull.hpp -- projection_hull_batch: the projection of a polytope {A x <= b} in R^d (d <= 16, at most 64 rows) onto
// k <= 3 of its coordinates by the iterative hull (polytope.py projection_iterhull, ref :1955-2100), for many polytopes in
// one launch, one polytope per wavefront (projhull_kernel, plp_projhull.hip).
// This header is the rule, compiled for the host (g++ -ffp-contract=off, tests/cabi/projhull_host.cpp) and for the device.
// It is a step function on a fixed-array state: step() runs until it needs something from outside, says what in
// State::req, and is called again once the answer stands in the state:
//   REQ_LP     max dir . x_keep over the polytope -> lp_status (LP_*), lp_x[d] (a point of the polytope that attains
//              it), lp_viol = max_i (a_i . x - b_i) of that point on the rows the LP ran on;
//   REQ_ENUM   the facets of the points held (enumerate(): the hullenum rule on the frame below; the kernel runs the same
//              candidates 64 at a time) -> count, fnu, foff, fon, en_flat, en_over;
//   REQ_DONE   status (PH_*) and the lists are final.
// The kernel and the host build share every decision; only who answers differs.
//
// The sequential contract:
//   box     the 2k LPs max +e_j, max -e_j over the kept coordinates j, in that order.  An unbounded one: PH_UNBOUNDED (a
//           bounded box is a bounded projection: unboundedness is decided here and nowhere else).  The projections of the
//           2k points give the FRAME: c = the centre of their coordinate ranges, s = the largest |p - c|_inf -- what
//           hullenum's staging computes from them, and, as they are the extremes of every coordinate, from every later
//           point list too (an LP point may leave the box by a rounding error: the frame stays the box's).  s not a
//           positive finite number: PH_FLAT.  q = (p - c) / s; every tolerance below is absolute on q.  The points then
//           join the list V in that order.
//   points  a new point is dropped when it is within SAME_TOL (max-norm on q) of one already held; a 65th point is
//           PH_OVERFLOW_POINTS.
//   rank    while V has fewer than k + 1 points or its enumeration is flat (a CAND_FLAT candidate, or no facet at all):
//           b_1, b_2, ... = Gram-Schmidt of the q_i - q_0, each time taking the point with the largest residual (the first
//           on a tie) while that residual exceeds SIDE_TOL; nu = the residual of the coordinate vector e_j with the
//           largest residual (the first on a tie) against the b, normalised.  Solve +nu and -nu; the point further from
//           the span (|nu . (q - q_0)|, +nu on a tie) joins V.  No point further than CONF_TOL: PH_FLAT.  A
//           full-dimensional polytope raises the rank every time; more than k passes: PH_FLAT.
//   rounds  enumerate the facets of V.  A facet that is `same` as one CONFIRMED before stays confirmed (confirmed facets
//           are supporting planes of the projection, so they remain facets while V grows; the frame does not move, so
//           the memo is compared on q).  Every other facet, in list order: the LP max nu . x_keep, h = nu . q of its point;
//           h <= off + CONF_TOL confirms the facet, otherwise the point joins V (subject to the dedupe).  A round that
//           adds no point ends the rule: the list is the answer.  Otherwise enumerate again.
//   LPs     an LP status other than optimal or unbounded, an unbounded LP after the box, or a point with
//           lp_viol > feas_tol (1e-9 max(1, |b|_max), as plp_support.hpp checks its points): PH_LPFAIL.  The (max_lps+1)-th
//           LP is not asked: PH_BUDGET.  Every loop is bounded by max_lps, MAX_POINTS or k.
// Tolerances.  SAME_TOL and SIDE_TOL are hullenum's (1e-9).  CONF_TOL = 1e-8 is derived, not measured: it must be at least
// SIDE_TOL, so that a point that is added is never "on" the facet it escaped and every round makes progress, and it is ten
// times below the 1e-7 at which the reference's own stop test (P1.contains(Vert, abs_tol)) gives up.
// Outputs (finish()): the rows of the accepted facets in the caller's coordinates (unit normals), their incidence words,
// V, and vmask: bit i set when point i lies on at least k accepted facets -- ADVISORY: a near-duplicate tilted row of one
// face (plp_hull_enum.hpp) can set the bit of a point inside an edge.  Rows are written for PH_OK only.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "plp_hull_enum.hpp"

namespace plp {
namespace projhull {

// the caps
constexpr int MAX_K = 3;                          // kept coordinates
constexpr int MAX_D = 16;                         // d
constexpr int MAX_ROWS = 64;                      // rows: one per lane
constexpr int MAX_POINTS = hullenum::MAX_POINTS;  // 64
constexpr int F_CAP = 128;                        // f_max <= F_CAP (the upper-bound theorem for 64 points in R^3: 124)
constexpr double CONF_TOL = 1e-8;
constexpr double SAME_TOL = hullenum::SAME_TOL, SIDE_TOL = hullenum::SIDE_TOL;
constexpr double FEAS_REL = 1e-9;                 // feas_tol = FEAS_REL max(1, |b|_max)

enum Status : int {   // include/plp.h: PLP_PH_*
    PH_OK = 0,
    PH_UNBOUNDED = 1,
    PH_FLAT = 2,
    PH_OVERFLOW_POINTS = 3,
    PH_OVERFLOW_FACETS = 4,
    PH_BUDGET = 5,
    PH_LPFAIL = 6,
    PH_NOCENTRE = 7   // (set by the callers: no strictly interior point was given; the rule never ran)
};
enum : int { REQ_DONE = 0, REQ_LP = 1, REQ_ENUM = 2 };
enum : int { LP_OPT = 0, LP_UNBND = 3 };   // the engine's ST_OPT / ST_UNBND; anything else fails
enum : int { P_START = 0, P_BOX, P_ENUM, P_RANK_PLUS, P_RANK_MINUS, P_ROUND };

template <int K>
struct State {
    // ---- set by begin()
    int d, f_max, max_lps;
    int keep[K];
    double feas_tol;
    // ---- the frame
    double c[K], s;
    // ---- the points: caller's coordinates, staged, and the identity index list candidate() wants
    int nv;
    double V[MAX_POINTS * K], q[MAX_POINTS * K];
    int sidx[MAX_POINTS];
    // ---- the facets of the last enumeration, on the frame
    int count, en_flat, en_over;
    double fnu[F_CAP * K], foff[F_CAP];
    uint64_t fon[F_CAP];
    uint64_t fconf[(F_CAP + 63) / 64];
    // ---- the facets confirmed so far (append-only)
    int nmemo;
    double mnu[F_CAP * K], moff[F_CAP];
    // ---- the request and the LP's answer
    int req;
    double dir[K];
    int lp_status;
    double lp_x[MAX_D], lp_viol;
    // ---- where the rule stands
    int phase, it, added, rank_passes, nrank, nlp, status;
    double box_x[2 * K][MAX_D], rank_x[MAX_D], rank_dist;
};

template <int K>
PLP_ENUM_FN void begin(State<K>& S, const int d, const int* keep, const int f_max, const int max_lps, const double b_absmax) {
    S.d = d;
    S.f_max = f_max < F_CAP ? f_max : F_CAP;
    S.max_lps = max_lps;
    for (int j = 0; j < K; ++j) S.keep[j] = keep[j];
    S.feas_tol = FEAS_REL * fmax(1.0, b_absmax);
    S.s = 0.0;
    for (int j = 0; j < K; ++j) S.c[j] = 0.0;
    S.nv = S.count = S.en_flat = S.en_over = S.nmemo = 0;
    for (int w = 0; w < (F_CAP + 63) / 64; ++w) S.fconf[w] = 0;
    S.req = REQ_DONE;
    S.lp_status = -1;
    S.lp_viol = 0.0;
    S.phase = P_START;
    S.it = S.added = S.rank_passes = S.nrank = S.nlp = 0;
    S.status = PH_OK;
    S.rank_dist = 0.0;
}

template <int K>
PLP_ENUM_FN int done(State<K>& S, const int status) {
    S.status = status;
    S.req = REQ_DONE;
    return REQ_DONE;
}
template <int K>
PLP_ENUM_FN int ask_lp(State<K>& S, const int phase) {
    if (S.nlp >= S.max_lps) return done(S, PH_BUDGET);
    S.nlp += 1;
    S.phase = phase;
    S.req = REQ_LP;
    return REQ_LP;
}
// the answer of the LP: 0 a point, 1 unbounded, 2 failed
template <int K>
PLP_ENUM_FN int lp_kind(const State<K>& S) {
    if (S.lp_status == LP_UNBND) return 1;
    if (S.lp_status != LP_OPT) return 2;
    return S.lp_viol <= S.feas_tol ? 0 : 2;   // (a NaN violation fails)
}
template <int K>
PLP_ENUM_FN void stage_point(const State<K>& S, const double* x, double (&p)[K], double (&qs)[K]) {
    for (int j = 0; j < K; ++j) {
        p[j] = x[S.keep[j]];
        qs[j] = (p[j] - S.c[j]) / S.s;
    }
}
// 1: joined V; 0: dropped as a duplicate; -1: a 65th point
template <int K>
PLP_ENUM_FN int add_point(State<K>& S, const double (&p)[K], const double (&qs)[K], const double* x, double* Xo) {
    for (int i = 0; i < S.nv; ++i) {
        bool close = true;
        for (int j = 0; j < K; ++j) close = close & (fabs(qs[j] - S.q[i * K + j]) <= SAME_TOL);
        if (close) return 0;
    }
    if (S.nv == MAX_POINTS) return -1;
    const int i = S.nv;
    for (int j = 0; j < K; ++j) {
        S.V[i * K + j] = p[j];
        S.q[i * K + j] = qs[j];
    }
    S.sidx[i] = i;
    if (Xo)
        for (int t = 0; t < S.d; ++t) Xo[(size_t)i * S.d + t] = x[t];
    S.nv = i + 1;
    return 1;
}

// the unit direction orthogonal to the affine span of the staged points (see "rank" above)
template <int K>
PLP_ENUM_FN void rank_direction(const State<K>& S, double (&nu)[K]) {
    double basis[K][K];
    int r = 0;
    while (r < K - 1) {
        int best = -1;
        double bestn = SIDE_TOL, bv[K];
        for (int j = 0; j < K; ++j) bv[j] = 0.0;
        for (int i = 1; i < S.nv; ++i) {
            double v[K];
            for (int j = 0; j < K; ++j) v[j] = S.q[i * K + j] - S.q[j];
            for (int t = 0; t < r; ++t) {
                const double g = wenum::dot<K>(v, basis[t]);
                for (int j = 0; j < K; ++j) v[j] = v[j] - g * basis[t][j];
            }
            const double n = sqrt(wenum::dot<K>(v, v));
            if (n > bestn) {
                bestn = n;
                best = i;
                for (int j = 0; j < K; ++j) bv[j] = v[j];
            }
        }
        if (best < 0) break;
        for (int j = 0; j < K; ++j) basis[r][j] = bv[j] / bestn;
        ++r;
    }
    double bestn = -1.0;
    for (int e = 0; e < K; ++e) {
        double v[K];
        for (int j = 0; j < K; ++j) v[j] = j == e ? 1.0 : 0.0;
        for (int t = 0; t < r; ++t) {
            const double g = wenum::dot<K>(v, basis[t]);
            for (int j = 0; j < K; ++j) v[j] = v[j] - g * basis[t][j];
        }
        const double n = sqrt(wenum::dot<K>(v, v));
        if (n > bestn) {
            bestn = n;
            for (int j = 0; j < K; ++j) nu[j] = v[j];
        }
    }
    for (int j = 0; j < K; ++j) nu[j] = nu[j] / bestn;   // (bestn >= 1 / sqrt(K): r < K)
}

template <int K>
PLP_ENUM_FN bool confirmed(const State<K>& S, const int f) { return (S.fconf[f >> 6] >> (f & 63)) & 1ull; }
template <int K>
PLP_ENUM_FN void confirm(State<K>& S, const int f) {
    S.fconf[f >> 6] |= 1ull << (f & 63);
    if (S.nmemo < F_CAP) {   // (a full memo only costs LPs)
        for (int j = 0; j < K; ++j) S.mnu[S.nmemo * K + j] = S.fnu[f * K + j];
        S.moff[S.nmemo] = S.foff[f];
        S.nmemo += 1;
    }
}

// The sequential enumeration of the facets of the points held: hullenum's candidates and greedy list on the frame
// (the twin of the kernel's rounds of 64 candidates).
template <int K>
PLP_ENUM_FN void enumerate(State<K>& S) {
    double nu[K], off = 0.0;
    uint64_t w = 0;
    bool flat = false;
    int count = 0;
    const bool over = wenum::greedy_list<K>(
        S.nv, S.f_max, count,
        [&](const int(&idx)[K]) {
            const int kind = hullenum::candidate<K>(S.q, S.sidx, S.nv, idx, nu, off, w);
            if (kind == hullenum::CAND_FLAT) flat = true;
            return kind == hullenum::CAND_FLAT ? wenum::LIST_END : (kind == hullenum::CAND_FACET ? wenum::LIST_TAKE : wenum::LIST_SKIP);
        },
        [&](const int f) { return hullenum::same<K>(nu, off, S.fnu + f * K, S.foff[f]); },
        [&](const int f, const int(&)[K]) {
            for (int j = 0; j < K; ++j) S.fnu[f * K + j] = nu[j];
            S.foff[f] = off;
            S.fon[f] = w;
        });
    S.count = count;
    S.en_flat = flat ? 1 : 0;
    S.en_over = over ? 1 : 0;
}

// Runs the rule until it needs an answer -> REQ_*.  Xo[64][d] or nullptr: the LP point above every entry of V.
template <int K>
PLP_ENUM_FN int step(State<K>& S, double* Xo) {
    int go = 0;   // what to do next without an answer: 1 enumerate (or rank), 2 rank, 3 the next facet of the round
    switch (S.phase) {
        case P_START:
            S.it = 0;
            for (int j = 0; j < K; ++j) S.dir[j] = j == 0 ? 1.0 : 0.0;
            return ask_lp(S, P_BOX);
        case P_BOX: {
            const int kind = lp_kind(S);
            if (kind == 1) return done(S, PH_UNBOUNDED);
            if (kind == 2) return done(S, PH_LPFAIL);
            for (int t = 0; t < S.d; ++t) S.box_x[S.it][t] = S.lp_x[t];
            S.it += 1;
            if (S.it < 2 * K) {
                for (int j = 0; j < K; ++j) S.dir[j] = j == (S.it >> 1) ? ((S.it & 1) ? -1.0 : 1.0) : 0.0;
                return ask_lp(S, P_BOX);
            }
            // the frame, then the 2k points in order
            double lo[K], hi[K];
            for (int j = 0; j < K; ++j) {
                lo[j] = __builtin_inf();
                hi[j] = -__builtin_inf();
                for (int i = 0; i < 2 * K; ++i) {
                    lo[j] = fmin(lo[j], S.box_x[i][S.keep[j]]);
                    hi[j] = fmax(hi[j], S.box_x[i][S.keep[j]]);
                }
                S.c[j] = hullenum::centre(lo[j], hi[j]);
            }
            double s = 0.0;
            for (int i = 0; i < 2 * K; ++i) {
                double p[K];
                for (int j = 0; j < K; ++j) p[j] = S.box_x[i][S.keep[j]];
                s = fmax(s, hullenum::reach<K>(p, S.c));
            }
            S.s = s;
            if (!(s > 0.0 && s < __builtin_inf())) return done(S, PH_FLAT);
            for (int i = 0; i < 2 * K; ++i) {
                double p[K], qs[K];
                stage_point(S, S.box_x[i], p, qs);
                add_point(S, p, qs, S.box_x[i], Xo);   // (2k <= 6 points: no overflow)
            }
            go = 1;
            break;
        }
        case P_ENUM:
            if (S.en_over) return done(S, PH_OVERFLOW_FACETS);
            if (S.en_flat || S.count == 0) {
                go = 2;
                break;
            }
            for (int w = 0; w < (F_CAP + 63) / 64; ++w) S.fconf[w] = 0;
            for (int f = 0; f < S.count; ++f) {
                double nu[K];
                for (int j = 0; j < K; ++j) nu[j] = S.fnu[f * K + j];
                bool hit = false;
                for (int t = 0; t < S.nmemo && !hit; ++t) hit = hullenum::same<K>(nu, S.foff[f], S.mnu + t * K, S.moff[t]);
                if (hit) S.fconf[f >> 6] |= 1ull << (f & 63);
            }
            S.it = 0;
            S.added = 0;
            go = 3;
            break;
        case P_RANK_PLUS:
        case P_RANK_MINUS: {
            if (lp_kind(S) != 0) return done(S, PH_LPFAIL);
            double p[K], qs[K], r[K];
            stage_point(S, S.lp_x, p, qs);
            for (int j = 0; j < K; ++j) r[j] = qs[j] - S.q[j];
            // dir = +-nu: |dir . (q - q_0)| either way
            const double dist = S.nv ? fabs(wenum::dot<K>(S.dir, r)) : 0.0;
            if (S.phase == P_RANK_PLUS) {
                S.rank_dist = dist;
                for (int t = 0; t < S.d; ++t) S.rank_x[t] = S.lp_x[t];
                for (int j = 0; j < K; ++j) S.dir[j] = -S.dir[j];
                return ask_lp(S, P_RANK_MINUS);
            }
            const bool minus = dist > S.rank_dist;
            const double best = minus ? dist : S.rank_dist;
            if (!(best > CONF_TOL)) return done(S, PH_FLAT);
            const double* x = minus ? S.lp_x : S.rank_x;
            stage_point(S, x, p, qs);
            const int a = add_point(S, p, qs, x, Xo);
            if (a < 0) return done(S, PH_OVERFLOW_POINTS);
            if (a == 0) return done(S, PH_FLAT);
            S.nrank += 1;
            go = 1;
            break;
        }
        case P_ROUND: {
            if (lp_kind(S) != 0) return done(S, PH_LPFAIL);
            double p[K], qs[K];
            stage_point(S, S.lp_x, p, qs);
            const double h = wenum::dot<K>(S.dir, qs);
            if (h <= S.foff[S.it] + CONF_TOL) {
                confirm(S, S.it);
            } else {
                const int a = add_point(S, p, qs, S.lp_x, Xo);
                if (a < 0) return done(S, PH_OVERFLOW_POINTS);
                S.added += a;
            }
            S.it += 1;
            go = 3;
            break;
        }
        default: return done(S, PH_LPFAIL);
    }
    if (go == 1) {
        if (S.nv >= K + 1) {
            S.phase = P_ENUM;
            S.req = REQ_ENUM;
            return REQ_ENUM;
        }
        go = 2;
    }
    if (go == 2) {
        S.rank_passes += 1;
        if (S.rank_passes > K || S.nv < 1) return done(S, PH_FLAT);
        rank_direction(S, S.dir);
        return ask_lp(S, P_RANK_PLUS);
    }
    // go == 3: the next facet of this round that is not confirmed
    while (S.it < S.count && confirmed(S, S.it)) S.it += 1;
    if (S.it < S.count) {
        for (int j = 0; j < K; ++j) S.dir[j] = S.fnu[S.it * K + j];
        return ask_lp(S, P_ROUND);
    }
    if (S.added == 0) return done(S, PH_OK);
    S.phase = P_ENUM;
    S.req = REQ_ENUM;
    return REQ_ENUM;
}

// The outputs of one polytope from its final state, entries [from, ..) in steps of `stride` (the host: 0, 1; the kernel:
// lane, 64).  Ao[f_max][K], bo[f_max], on[f_max], Vo[64][K]; f_max is the caller's (<= F_CAP).
template <int K>
PLP_ENUM_FN int out_count(const State<K>& S) { return S.status == PH_OK ? S.count : 0; }
template <int K>
PLP_ENUM_FN void finish_rows(const State<K>& S, const int f_max, double* Ao, double* bo, uint64_t* on, const int from,
                             const int stride) {
    const int cnt = out_count(S);
    for (int f = from; f < f_max; f += stride) {
        const bool in = f < cnt;
        for (int j = 0; j < K; ++j) Ao[(size_t)f * K + j] = in ? S.fnu[f * K + j] : __builtin_nan("");
        bo[f] = in ? hullenum::unstage<K>(S.fnu + f * K, S.foff[f], S.c, S.s) : __builtin_nan("");
        on[f] = in ? S.fon[f] : 0;
    }
}
template <int K>
PLP_ENUM_FN void finish_points(const State<K>& S, double* Vo, double* Xo, const int from, const int stride) {
    for (int i = from; i < MAX_POINTS; i += stride) {
        const bool in = i < S.nv;
        for (int j = 0; j < K; ++j) Vo[(size_t)i * K + j] = in ? S.V[i * K + j] : __builtin_nan("");
        if (Xo && !in)
            for (int t = 0; t < S.d; ++t) Xo[(size_t)i * S.d + t] = __builtin_nan("");
    }
}
// point i lies on at least K accepted facets
template <int K>
PLP_ENUM_FN bool vertex_bit(const State<K>& S, const int i) {
    const int cnt = out_count(S);
    int hits = 0;
    for (int f = 0; f < cnt; ++f) hits += (int)((S.fon[f] >> i) & 1ull);
    return i < S.nv && hits >= K;
}
template <int K>
PLP_ENUM_FN uint64_t vertex_mask(const State<K>& S) {
    uint64_t mask = 0;
    for (int i = 0; i < S.nv; ++i) mask |= (uint64_t)vertex_bit<K>(S, i) << i;
    return mask;
}

}  // namespace projhull
}  // namespace plp
