/*
 * plp.h -- C ABI of libplp_hip.so: the MI355X (gfx950) engine for the batched small-LP hot
 * path of tulip-control/polytope.  Plain pointers and sizes only; no torch / C++ types.
 *
 * The reference is pure Python and has no FFI of its own; the boundary this library sits
 * behind is the reference's solver plug-in surface and the numpy kernels listed below
 * (paths relative to the reference checkout).  Each entry point cites what it replaces.
 *
 * Conventions
 *   - all floating point data is IEEE binary64 ("double"), C-contiguous, caller-owned;
 *     nothing is retained after a call returns (reduce() passes aliases of arrays it
 *     mutates around the call: polytope/polytope.py:1146-1151).
 *   - a batch of polytopes is packed as A[B][m_max][d], b[B][m_max] with an optional
 *     int32 m[B] (rows actually used, <= m_max; NULL = all m_max).  d <= 16.  m_max <= 64 for the fused
 *     kernels (reduce, bounding boxes, pair LPs: register-resident dictionaries); plp_lp_solve_batch and
 *     plp_cheby_batch also take m_max > 64 -- region_diff stacks m_poly + sum(active rows) without a limit
 *     (polytope/polytope.py:2212-2224) -- as long as one dictionary fits the CU's 160 KB of LDS
 *     (about 890 rows at n = 17, 3000 at n = 4); beyond that PLP_EUNSUPPORTED.
 *   - per-LP status codes are scipy.optimize.linprog's, as returned by
 *     polytope.solvers.lpsolve (polytope/solvers.py:76-106, 155-158):
 *        0 optimal, 1 iteration limit, 2 infeasible, 3 unbounded, 4 numerical trouble.
 *     An LP that fails is NOT an error of the call: it is status != 0 with x/fun = NaN.
 *   - function return value: PLP_OK, or PLP_E* for API misuse / HIP errors
 *     (plp_last_error() has the text).  Nothing throws across this boundary.
 *   - "_dev" variants take DEVICE pointers and a HIP stream (void* = hipStream_t, NULL =
 *     default stream), enqueue the work and return without synchronising.  Every launch,
 *     memset and copy of a "_dev" call goes to `stream`, and the host does not wait for any
 *     of it: the results are ordered like any other work on that stream.  (A scratch buffer
 *     of the context that has to grow is freed after its last user has finished: the call
 *     then waits for that work, on `stream` or, for the one buffer the streams share, on the
 *     stream that used it last; a 17th stream on one context waits for the device once.)
 *     The plain variants take HOST pointers, copy in/out through the context's scratch
 *     buffers and block until results are host-visible.
 *   - a plp_ctx is not thread safe; use one per thread (the reference is single-threaded).
 */
#ifndef PLP_H
#define PLP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PLP_OK 0
#define PLP_EINVAL 1       /* bad argument (NULL pointer, negative size, ...)            */
#define PLP_EUNSUPPORTED 2 /* size outside the engine's envelope (d > 16, too many rows)  */
#define PLP_EHIP 3         /* HIP runtime error                                          */
#define PLP_ENODEVICE 4    /* no gfx950 device visible                                   */
#define PLP_ENONFINITE 5   /* an input held inf or nan (only with plp_ctx_set_check_finite) */

/* flags[] bits written by plp_reduce_batch (see polytope/polytope.py:1053-1163) */
#define PLP_RF_EMPTY 1  /* not full-dimensional: reduce() returns Polytope()       (:1081-1082) */
#define PLP_RF_EARLY 2  /* returned at neq <= nx+1, minrep stays False             (:1114-1116, :1136-1138) */
#define PLP_RF_MINREP 4 /* all redundancy LPs done, minrep = True                  (:1161-1163) */
#define PLP_RF_LPFAIL 8 /* a bounding-box LP ended 1/4: reference raises RuntimeError (:1378-1384) */
/* set beside PLP_RF_EMPTY when the verdict is the ENGINE's, not the polytope's: the fused kernel's Chebyshev LP ended neither
 * optimal nor infeasible, or "optimal" at a centre that violates a row (rows a hair apart).  The fused reduce is not verified:
 * ask plp_cheby_batch (verified) about such a polytope, as polytope_amd.polytope.reduce does. */
#define PLP_RF_F1OPEN 32

typedef struct plp_ctx plp_ctx;

int plp_version(void);
/* number of visible HIP devices whose architecture is gfx950 (0 if none / no runtime) */
int plp_device_count(void);
const char *plp_last_error(void);

int plp_ctx_create(int device, plp_ctx **out);
/* on != 0: the host-pointer entry points plp_lp_solve_batch / plp_cheby_batch / plp_bbox_batch / plp_reduce_batch return
 * PLP_ENONFINITE, writing no output, when c / G / h resp. A / b hold an inf or a nan -- the ValueError
 * scipy.optimize.linprog raises for such input behind solvers.lpsolve (solvers.py:152-154).  Large batches are checked
 * by the threads that stage them for upload, at no extra pass over the data.  Off by default: the kernels then report
 * such LPs with status 4. */
int plp_ctx_set_check_finite(plp_ctx *ctx, int on);
int plp_ctx_destroy(plp_ctx *ctx);
/* block until everything enqueued on `stream` (NULL = default stream) has finished */
int plp_ctx_synchronize(plp_ctx *ctx, void *stream);

/*
 * Batched lpsolve():  B independent LPs   min c'x  s.t.  G x <= h,  x free.
 * Replaces: polytope.solvers.lpsolve / _solve_lp_using_scipy
 *           (polytope/solvers.py:76-106, :149-158) called in Python loops at
 *           polytope/polytope.py:1150, :1288, :1371, :1393.
 * c[B][n], G[B][m_max][n], h[B][m_max], m[B] or NULL;  n <= 17.  m_max > 64: LDS-resident engine.
 * Out: x[B][n], fun[B] (NaN unless status 0), status[B], iters[B] (may be NULL).
 */
int plp_lp_solve_batch(plp_ctx *ctx, int64_t B, int m_max, int n, const double *c, const double *G,
                       const double *h, const int32_t *m, double *x, double *fun, int32_t *status,
                       int32_t *iters);
int plp_lp_solve_batch_dev(plp_ctx *ctx, void *stream, int64_t B, int m_max, int n, const double *c,
                           const double *G, const double *h, const int32_t *m, double *x, double *fun,
                           int32_t *status, int32_t *iters);

/*
 * Batched Chebyshev ball, LP form F1:  max r  s.t.  a_i.x + ||a_i|| r <= b_i.
 * Replaces: cheby_ball (polytope/polytope.py:1241-1300; G,h,c built at :1283-1287) and
 *           therefore is_fulldim (:962-985).
 * Out: r[B] = x[-1] of the LP (may be negative: the caller applies ":1291 r < 0 -> empty"),
 *      xc[B][d], status[B] raw LP status.
 */
int plp_cheby_batch(plp_ctx *ctx, int64_t B, int m_max, int d, const double *A, const double *b,
                    const int32_t *m, double *r, double *xc, int32_t *status);
int plp_cheby_batch_dev(plp_ctx *ctx, void *stream, int64_t B, int m_max, int d, const double *A,
                        const double *b, const int32_t *m, double *r, double *xc, int32_t *status);

/*
 * Bounding boxes of a batch of polytopes (1 <= d <= 16, m_max <= 64): per polytope the Chebyshev LP and then the 2d LPs
 * min +-e_i.x (form F3) started from its centre -- one launch instead of 2d generic LPs per polytope (d > 8, and
 * d = 5..8 with more than 32 rows in batches beyond 1024 polytopes: one polytope per wavefront, every LP with a
 * wave-uniform pivot; d >= 14: the 2d LPs without a stored dictionary).
 * Replaces: the LP loops of bounding_box (polytope/polytope.py:1367-1409).
 * Out: lb[B][d], ub[B][d] (-inf / +inf where the LP is unbounded, :1376 / :1398) and status[B]:
 *      0 = lb/ub hold the box,
 *      1 = not handled here (no Chebyshev centre with r >= 1e-6: empty, flat or unbounded-ball polytopes; LPs that
 *          need Bland's rule, for d > 8 also LPs of more than 32 pivots): lb/ub are NaN and the caller solves the 2d generic LPs (plp_lp_solve_batch), whose
 *          statuses 2 / 3 then take the reference's branches (:1378-1380, :1400-1402).
 */
int plp_bbox_batch(plp_ctx *ctx, int64_t B, int m_max, int d, const double *A, const double *b, const int32_t *m,
                   double *lb, double *ub, int32_t *status);
int plp_bbox_batch_dev(plp_ctx *ctx, void *stream, int64_t B, int m_max, int d, const double *A, const double *b,
                       const int32_t *m, double *lb, double *ub, int32_t *status);

/*
 * Fused reduce() of a batch of polytopes (none of them minrep):  F1, parallel-row dedupe,
 * bounding-box prefilter (2d LPs F3, when rows > 3d) and one redundancy LP F2 per row.
 * Replaces: reduce (polytope/polytope.py:1053-1163), including the is_fulldim/cheby_ball
 *           call at :1081 and the bounding_box call at :1119 (:1314-1411).
 * Out: keep[B]  bit i set <=> input row i is kept;
 *      flags[B] PLP_RF_* ;  r[B], xc[B][d] the Chebyshev ball of the INPUT polytope
 *      (r = 0, xc = NaN when cheby_ball would return (0, None));
 *      nlp[B]   number of LPs the reference would have issued (= LPs solved here).
 */
int plp_reduce_batch(plp_ctx *ctx, int64_t B, int m_max, int d, const double *A, const double *b,
                     const int32_t *m, double abs_tol, uint64_t *keep, int32_t *flags, double *r,
                     double *xc, int32_t *nlp);
int plp_reduce_batch_dev(plp_ctx *ctx, void *stream, int64_t B, int m_max, int d, const double *A,
                         const double *b, const int32_t *m, double abs_tol, uint64_t *keep,
                         int32_t *flags, double *r, double *xc, int32_t *nlp);

/*
 * In-run accounting of plp_reduce_batch[_dev]: nlp[] counts the LPs the REFERENCE issues for a polytope
 * (polytope/polytope.py:1081, :1119, :1142-1151: 1 + 2d + one per row that reaches the redundancy loop).  Not all of them
 * run the simplex here: a redundancy LP whose verdict "keep" a feasible witness point proves (the presolve)
 * is answered without one.  This call returns the number of LPs that DID run the simplex in the fused reduce launches
 * issued through `ctx` since the counter was last reset (all streams; the first call of a context switches the counting
 * on and returns 0).  It enqueues a copy on `stream` and blocks until it has landed, so it sees every launch enqueued on
 * that stream before it.  reset != 0: the counter restarts at zero.  The second pass that redoes polytopes flagged for
 * Bland's rule and the kernels for more than 64 rows do not count.
 */
int plp_reduce_counters(plp_ctx *ctx, void *stream, uint64_t *simplex_runs, int reset);

/*
 * The verifier behind plp_lp_solve_batch / plp_cheby_batch / plp_bbox_batch (round 6; csrc/plp_verify.hpp says why): every
 * answer of the LP engines is certified against the original rows from its final basis -- its vertex recomputed, its
 * multipliers' signs checked, every row tested -- and what does not certify (or is reported unbounded / at a limit) is
 * solved again by a careful double-double engine.  This call returns, for the LAST verified batch issued on `stream`
 * through `ctx`, how many of its LPs went to the careful engine (0 on random, ragged, rescaled, flat or lattice data;
 * ~5 % of the LPs of polytopes with rows 1e-16 .. 1e-5 rad apart; every unbounded LP).  It blocks until that batch is done.
 * PLP_VERIFY=0 in the environment switches the verifier off (A/B measurements: the answers then are the engines' own).
 */
int plp_verify_counters(plp_ctx *ctx, void *stream, int64_t *careful_lps);

/*
 * The same for polytopes of ANY row count whose rows and dictionary fit the LDS of a CU (about 500 rows at d = 16,
 * 2000 at d = 3): `reduce` has no row limit in the reference (polytope/polytope.py:1053-1163), Polytope.intersect
 * stacks m1 + m2 rows (:268-275) and region_diff's leaves as many as the search collected (:2276).
 * keep[B][W], W = (m_max + 63) / 64 words per polytope, bit i of word i / 64 <=> input row i is kept; everything else
 * as plp_reduce_batch (to which m_max <= 64 is passed on, W = 1).  PLP_EUNSUPPORTED when a polytope does not fit.
 */
int plp_reduce_wide_batch(plp_ctx *ctx, int64_t B, int m_max, int d, const double *A, const double *b,
                          const int32_t *m, double abs_tol, uint64_t *keep, int32_t *flags, double *r,
                          double *xc, int32_t *nlp);
int plp_reduce_wide_batch_dev(plp_ctx *ctx, void *stream, int64_t B, int m_max, int d, const double *A,
                              const double *b, const int32_t *m, double abs_tol, uint64_t *keep,
                              int32_t *flags, double *r, double *xc, int32_t *nlp);

/*
 * One Fourier-Motzkin elimination step of projection(solver="fm") (polytope/polytope.py:1911-1952) for B packed
 * polytopes, fused with the compaction of the reduce() that produced their rows.
 * In:  A[B][m_max][d], b[B][m_max], m[B] (NULL = m_max) as for plp_reduce_batch;
 *      keep[B][kw] (NULL = every row) and flags[B] (NULL = none) of the plp_reduce_batch / plp_reduce_wide_batch call
 *      that produced the rows: only rows whose keep bit is set are read; with flags, each such row gets what
 *      reduce() does to it on the way out (PLP_RF_MINREP: b = (b + 0.1) - 0.1; then one Polytope constructor pass:
 *      scale by the reciprocal norm, rows of norm <= 1e-10 dropped); first != 0 adds one more constructor pass (the
 *      copy() of the first step, :1923); polytopes flagged PLP_RF_EMPTY / PLP_RF_LPFAIL / 32 (re-examine) have no rows.
 *      col: the column eliminated (0 <= col < d, d >= 2); col < 0: no elimination, the staged rows themselves.
 * plp_fm_count: count[B] = |N| + |P| |Q| with P: a_col > abs_tol, Q: a_col < -abs_tol, N: |a_col| < abs_tol
 *      (a coefficient of exactly +-abs_tol: the row is dropped, :1925-1927).
 * plp_fm_emit: the rows, in the reference's order (P x Q with P major, then N), column col removed, each scaled by the
 *      constructor (rows of norm <= 1e-10 dropped), into A_out[B][mo_max][d_out], b_out[B][mo_max] (d_out = d - 1, or d
 *      for col < 0; rows from m_out[B] on are zero) and m_out[B]; m_out = -1: more than mo_max rows, nothing written.
 *      A combined row is  fma(a_j,col, x_k, (-a_k,col) * x_j)  element-wise, A and b alike.
 * The input of a polytope must fit the LDS of a CU: m_max (d + 1) 8 + 12 m_max <= 160 KB, else PLP_EUNSUPPORTED.
 */
int plp_fm_count(plp_ctx *ctx, int64_t B, int m_max, int d, const double *A, const double *b, const int32_t *m,
                 const uint64_t *keep, int kw, const int32_t *flags, int col, int first, double abs_tol,
                 int32_t *count);
int plp_fm_count_dev(plp_ctx *ctx, void *stream, int64_t B, int m_max, int d, const double *A, const double *b,
                     const int32_t *m, const uint64_t *keep, int kw, const int32_t *flags, int col, int first,
                     double abs_tol, int32_t *count);
int plp_fm_emit(plp_ctx *ctx, int64_t B, int m_max, int d, const double *A, const double *b, const int32_t *m,
                const uint64_t *keep, int kw, const int32_t *flags, int col, int first, double abs_tol, int mo_max,
                double *A_out, double *b_out, int32_t *m_out);
int plp_fm_emit_dev(plp_ctx *ctx, void *stream, int64_t B, int m_max, int d, const double *A, const double *b,
                    const int32_t *m, const uint64_t *keep, int kw, const int32_t *flags, int col, int first,
                    double abs_tol, int mo_max, double *A_out, double *b_out, int32_t *m_out);

/*
 * The hit counts of volume() (polytope/polytope.py:1529-1594, lines :1586-1591) for B packed polytopes: how many of
 * the N uniform samples of each polytope's bounding box lie strictly inside it.  The samples are the ones
 * numpy.random.default_rng(seed).random((d, N)) draws -- PCG64 (XSL-RR 128/64), element (i, j) at stream position
 * i * N + j -- generated on the device by exact jump-ahead: no sample crosses the bus.
 * In:  A[B][m_max][d], b[B][m_max], m[B] (NULL = m_max) as for plp_reduce_batch;
 *      lb[B][d], ub[B][d]: the boxes (plp_bbox_batch);
 *      state[B][2], inc[B][2]: per polytope the generator's 128-bit state and increment, low word first
 *      (numpy.random.PCG64(seed).state['state']);
 *      N: samples per polytope, 1 <= N <= 2^31 - 1 (else PLP_EINVAL).
 * Out: hits[B]: samples x = lb + r * (ub - lb) (a multiplication, then an addition) with (s - b_i) < 0 for every row i,
 *      s = a_i0 x_0 and then s = fma(a_ik, x_k, s) for k = 1 .. d - 1: plp_contains' arithmetic with abs_tol = 0, so the
 *      count is the one plp_contains gives on the uploaded samples.  The volume is prod(ub - lb) * hits / N.
 *      flags[B]: 0, or PLP_VF_NONFINITE (a bound of the box is inf / nan) | PLP_VF_NOROWS (m = 0): not sampled, hits = 0.
 * d <= 16 and m_max <= 64, else PLP_EUNSUPPORTED.
 */
#define PLP_VF_NONFINITE 1
#define PLP_VF_NOROWS 2
int plp_volume_hits(plp_ctx *ctx, int64_t B, int m_max, int d, const double *A, const double *b, const int32_t *m,
                    const double *lb, const double *ub, const uint64_t *state, const uint64_t *inc, int64_t N,
                    uint32_t *hits, int32_t *flags);
int plp_volume_hits_dev(plp_ctx *ctx, void *stream, int64_t B, int m_max, int d, const double *A, const double *b,
                        const int32_t *m, const double *lb, const double *ub, const uint64_t *state,
                        const uint64_t *inc, int64_t N, uint32_t *hits, int32_t *flags);

/*
 * Support functions  h_P(c) = max { c.x : A x <= b }  of B packed polytopes in K directions each (template directions,
 * H-in-H containment, the facet LPs of an iterative hull): the rows of a polytope are read once for all its directions.
 * In:  A[B][m_max][d], b[B][m_max], m[B] (NULL = m_max) as for plp_reduce_batch;
 *      C: the directions, [K][d] shared by every polytope (c_shared != 0) or [B][K][d];
 *      xc[B][d]: a STRICTLY interior point of each polytope (plp_cheby_batch's centre), from which every LP starts.
 * Out: val[B][K] = c.x at the optimum (the MAXIMUM), x[B][K][d] the point (NULL: not written), status[B][K]:
 *        0  optimum;
 *        3  unbounded in that direction: val = +inf, x = NaN;
 *        1  NOT SETTLED HERE (val = x = NaN) -- a row i < m with b_i - a_i.xc <= 0 (xc is not strictly inside, or NaN),
 *           an LP the one-LP-per-lane engine hands back (degenerate steps, dependent active rows, its iteration cap), or a
 *           final point x' = x - xc with  max_i (a_i.x' - beta_i) > 1e-9 max(1, |beta|_max),  beta_i = b_i - a_i.xc.  The
 *           caller solves these (polytope, direction) pairs as generic LPs (plp_lp_solve_batch with c = -C).
 *      That end check is a feasibility check only; optimality is the engine's own multiplier test.  The answers of this
 *      call are NOT under the verifier's certificate (plp_verify_counters does not see them).
 * d <= 4, m_max <= 64, K >= 1 and B * K <= 2^31 - 1, else PLP_EUNSUPPORTED.  B = 0: returns PLP_OK, nothing runs.
 * The host-pointer form checks A, b and C for inf / nan when the context asks for it (plp_ctx_set_check_finite).
 */
int plp_support_batch(plp_ctx *ctx, int64_t B, int m_max, int d, const double *A, const double *b, const int32_t *m,
                      int K, const double *C, int c_shared, const double *xc, double *val, double *x, int32_t *status);
int plp_support_batch_dev(plp_ctx *ctx, void *stream, int64_t B, int m_max, int d, const double *A, const double *b,
                          const int32_t *m, int K, const double *C, int c_shared, const double *xc, double *val,
                          double *x, int32_t *status);

/*
 * Nearest points and Euclidean distances:  min |x - p|_2  s.t.  A x <= b  for B packed polytopes and K points each -- a
 * strictly convex QP per (polytope, point), one dual active-set walk per lane, the rows of a polytope read once per
 * tile and chunk of its points.
 * In:  A[B][m_max][d], b[B][m_max], m[B] (NULL = m_max) as for plp_reduce_batch.  Rows are used at unit 2-norm; a zero row
 *      with b >= 0 is ignored, a zero row with b < 0 makes the polytope empty;
 *      X: the points, [K][d] shared by every polytope (x_shared != 0) or [B][K][d].
 * Out: dist[B][K] = |x - p|_2;  x[B][K][d] the nearest point (NULL: not written);
 *      face[B][K] (NULL ok): bit i set = row i is in the final active set (the keep-word convention);
 *      lam[B][K][d] (NULL ok): the multipliers of the set bits of face in ascending row order, with respect to the rows as
 *      given -- p - x = sum lam_j a_j -- zero-padded;  status[B][K]:
 *        0  optimum.  With E = max(1, |x|_inf, |p|_inf) the point passed  max_i (n_i.x - beta_i) <= 1e-10 E  on every row and a
 *           certificate on the rows of face: lam >= 0,  sum lam_j |beta_j - n_j.x| <= 1e-10 E max(dist, 1e-10 E),
 *           |(p - x) - sum lam_j n_j|_2 <= 1e-12 E  (unit rows).  For a feasible x that bounds |x - x*| by
 *           |r| + sqrt(|r|^2 + 2 gap) and dist - dist* by 2 (gap + |r| |x - x*|) / dist.  A point that violates no row comes
 *           back as x = p bit for bit, dist = 0, face = 0;
 *        2  the polytope is empty, certified by a Farkas combination y >= 0 on at most d + 1 rows with
 *           |sum y_j n_j|_1 <= 1e-12 sum y_j  and  sum y_j beta_j < -1e-10 sum y_j:  dist = x = NaN;
 *        1  NOT SETTLED HERE (dist = x = NaN, face = 0, lam = 0): the walk handed the problem back (nearly dependent active
 *           rows, a run of steps of length zero, its iteration cap 2 (m + 2 d) + 4), an end check or the Farkas check
 *           failed, or the point or a row of the polytope is not finite.  The caller settles these (polytope_amd.batch:
 *           nearest_batch(resolve=True) enumerates row subsets on the host).
 * d <= 4, m_max <= 64, K >= 1 and B * K <= 2^31 - 1, else PLP_EUNSUPPORTED.  B = 0: returns PLP_OK, nothing runs.
 * The host-pointer form checks A, b and X for inf / nan when the context asks for it (plp_ctx_set_check_finite).
 */
int plp_nearest_batch(plp_ctx *ctx, int64_t B, int m_max, int d, const double *A, const double *b, const int32_t *m,
                      int K, const double *X, int x_shared, double *dist, double *x, uint64_t *face, double *lam,
                      int32_t *status);
int plp_nearest_batch_dev(plp_ctx *ctx, void *stream, int64_t B, int m_max, int d, const double *A, const double *b,
                          const int32_t *m, int K, const double *X, int x_shared, double *dist, double *x, uint64_t *face,
                          double *lam, int32_t *status);

/*
 * Vertices of B packed polytopes (H-representation to V-representation on the small-polytope path): every d-subset of a
 * polytope's rows is solved and tested against all rows, one polytope per wavefront, the rows read once.
 * In:  A[B][m_max][d], b[B][m_max], m[B] (NULL = m_max) as for plp_reduce_batch;
 *      keep[B] (NULL = every row): bit i set = row i is live, the keep word of plp_reduce_batch.  Pass it: rows that are
 *      redundant to 1e-7 but not identical do cross somewhere, and each crossing inside the polytope is reported.
 * Rule (sequential; the kernel computes exactly this list): the live rows, scaled to unit 2-norm, in row order -- a live
 *      zero row with b >= 0 is ignored, with b < 0 the polytope is empty; every d-subset (i0 < i1 < ...) in lexicographic
 *      order, skipped when |det| <= 1e-12; the solution v is feasible when a_i.v - b_i <= 1e-9 max(1, |v|_inf, |b_i|) on
 *      every staged row; a feasible v is dropped when a vertex accepted BEFORE it lies within 1e-9 max(1, |v|_inf) of it
 *      in the max-norm.  Each geometric vertex appears once, whatever its degeneracy.
 * Out: V[B][v_max][d] the vertices in that order (NaN beyond count), count[B],
 *      basis[B][v_max][d] the ORIGINAL row indices of the accepting subset (-1 beyond count; NULL: not written), status[B]:
 *        0                all vertices written;
 *        PLP_XS_OVERFLOW  more than v_max distinct vertices: the first v_max are written, count = v_max;
 *        PLP_XS_EMPTY     no feasible candidate, or an infeasible zero row: count = 0.
 *      The caller vouches for boundedness: an unbounded polytope has the vertices the rule finds and no status of its own
 *      (PLP_XS_FLAT / PLP_XS_UNBOUNDED are set by callers that test for it first, as extreme_batch of the Python package does).
 * 1 <= d <= 4 and m_max <= 64, else PLP_EUNSUPPORTED; v_max < 1 is PLP_EINVAL.  B = 0: returns PLP_OK, nothing runs.
 * The host-pointer form checks A and b for inf / nan when the context asks for it (plp_ctx_set_check_finite).
 */
#define PLP_XS_OVERFLOW 1
#define PLP_XS_EMPTY 2
#define PLP_XS_FLAT 3      /* set by callers: empty or not full-dimensional (Chebyshev radius <= abs_tol) */
#define PLP_XS_UNBOUNDED 4 /* set by callers: a side of the bounding box is infinite                      */
int plp_extreme_batch(plp_ctx *ctx, int64_t B, int m_max, int d, const double *A, const double *b, const int32_t *m,
                      const uint64_t *keep, int v_max, double *V, int32_t *count, int32_t *basis, int32_t *status);
int plp_extreme_batch_dev(plp_ctx *ctx, void *stream, int64_t B, int m_max, int d, const double *A, const double *b,
                          const int32_t *m, const uint64_t *keep, int v_max, double *V, int32_t *count, int32_t *basis,
                          int32_t *status);

/*
 * Facets of B packed point sets (V-representation to H-representation on the small-set path, the other direction of
 * plp_extreme_batch): every d-subset of a set's points spans a hyperplane, which is a facet when all points lie on one
 * side of it; one point set per wavefront, the points read once.
 * In:  X[B][n_max][d], n[B] (NULL = n_max): the points in use per set;
 *      keep[B] (NULL = every point): bit i set = point i is live.
 * Rule (sequential; the kernel computes exactly this list): the live points in index order, moved to the centre
 *      c = (min + max) / 2 of their bounding box and divided by s = max |p_i - c|_inf, so that they lie in [-1, 1]^d and
 *      the tolerances are absolute.  Every d-subset (i0 < i1 < ...) in lexicographic order: nu = the generalised cross
 *      product of the edges q_ik - q_i0, skipped unless |nu| > 1e-12 prod |edges|; nu scaled to unit length,
 *      r_i = nu.(q_i - q_i0) over all points.  All |r_i| <= 1e-9: the set is flat.  max r <= 1e-9: the facet nu;
 *      min r >= -1e-9: the facet -nu.  A facet is dropped when one accepted BEFORE it has the same normal and offset to
 *      1e-9 (max-norm), so a face with more than d points appears once.
 * Out: Ao[B][f_max][d] unit normals and bo[B][f_max], the rows Ao x <= bo in the caller's coordinates, in that order (NaN
 *      beyond count); on[B][f_max]: bit i set = point i is live and lies on the facet to 1e-9 of the extent (0 beyond
 *      count); count[B]; basis[B][f_max][d] the ORIGINAL indices of the accepting subset (-1 beyond count; NULL: not
 *      written); status[B]:
 *        0                all facets written;
 *        PLP_HS_OVERFLOW  more than f_max distinct facets: the first f_max are written, count = f_max;
 *        PLP_HS_FLAT      fewer than d + 1 live points, all of them one point, or all on one hyperplane: count = 0.
 *      The rows are neither reduced nor ordered further; no vertex list is written (the bits of `on` are the points on
 *      the boundary, plp_extreme_batch on the rows gives the vertices).
 * 1 <= d <= 4 and n_max <= 64, else PLP_EUNSUPPORTED; f_max < 1 is PLP_EINVAL.  B = 0: returns PLP_OK, nothing runs.
 * The host-pointer form checks X for inf / nan when the context asks for it (plp_ctx_set_check_finite).
 */
#define PLP_HS_OK 0
#define PLP_HS_OVERFLOW 1
#define PLP_HS_FLAT 2
int plp_hull_batch(plp_ctx *ctx, int64_t B, int n_max, int d, const double *X, const int32_t *n, const uint64_t *keep,
                   int f_max, double *Ao, double *bo, uint64_t *on, int32_t *count, int32_t *basis, int32_t *status);
int plp_hull_batch_dev(plp_ctx *ctx, void *stream, int64_t B, int n_max, int d, const double *X, const int32_t *n,
                       const uint64_t *keep, int f_max, double *Ao, double *bo, uint64_t *on, int32_t *count,
                       int32_t *basis, int32_t *status);

/*
 * Exact volumes and facet areas of B packed polytopes (d <= 4): Lasserre's facet recursion on the rows,
 * vol_d(P) = (1 / d) sum_i h_i vol_{d-1}(P ^ H_i), taken down to lines where the measure is an interval length; no vertex
 * list, no LP, no samples.  One polytope per wavefront, the rows read once.
 * In:  A[B][m_max][d], b[B][m_max], m[B] (NULL = m_max) as for plp_reduce_batch;
 *      keep[B] (NULL = every row): bit i set = row i is live, the keep word of plp_reduce_batch;
 *      xc[B][d] (NULL = 0) and scale[B] (NULL = 1): the rule runs on the rows of (P - xc) / scale, on which its tolerances
 *      are absolute; a point inside the polytope and half the longest side of its bounding box keep them meaningful.
 * Rule (sequential; the kernel computes exactly these numbers, polytope_amd/csrc/plp_volume_exact.hpp): the live rows
 *      scaled to unit 2-norm, in row order -- a live zero row with b >= 0 is ignored, with b < 0 (or NaN) the member is
 *      empty.  A chain of rows (i_1 .. i_k) is the face on which they are tight, with an orthonormal basis of their normals
 *      and the foot point of the reference point on it.  A row whose normal, projected off the chain's, shrinks by 1e-12 at
 *      some level is parallel to the face there: more than 1e-9 behind it, the face is empty; on it to 1e-9, facing the same
 *      way and of lower index than the chain's row of that level, the face belongs to that row and this chain is empty;
 *      else the row says nothing.  The other rows cut the face; a full chain (d - 1 rows) is a line, cut to an interval.
 *      Sums over the cutting rows in increasing index.
 * Out: volume[B]; area[B][m_max] the (d-1)-measure of each row's facet at the row's index, 0 for rows that are not live
 *      (d = 1: 1 for the lowest-index row at each end; NULL: not written); status[B]:
 *        PLP_VS_OK         a volume of 0 is the answer for an empty or a flat set;
 *        PLP_VS_UNBOUNDED  volume = +inf: a face has no end, or no row cuts it (a member without rows included);
 *        PLP_VS_EMPTY      an infeasible zero row: volume 0, areas 0.
 *      (PLP_VS_FLAT is set by callers that test for it first, as volume_exact_batch of the Python package does.)
 * Cost: n^(d-1) chains of n rows each for n live rows -- as plp_extreme_batch at (16, 3), milliseconds per polytope at (64, 4).
 * 1 <= d <= 4 and m_max <= 64, else PLP_EUNSUPPORTED.  B = 0: returns PLP_OK, nothing runs, no pointer is touched.
 * The host-pointer form checks A, b, xc and scale for inf / nan when the context asks for it (plp_ctx_set_check_finite).
 */
#define PLP_VS_OK 0
#define PLP_VS_UNBOUNDED 1
#define PLP_VS_EMPTY 2
#define PLP_VS_FLAT 3 /* set by callers: empty or not full-dimensional (Chebyshev radius <= abs_tol) */
int plp_vol_exact_batch(plp_ctx *ctx, int64_t B, int m_max, int d, const double *A, const double *b, const int32_t *m,
                           const uint64_t *keep, const double *xc, const double *scale, double *volume, double *area,
                           int32_t *status);
int plp_vol_exact_batch_dev(plp_ctx *ctx, void *stream, int64_t B, int m_max, int d, const double *A, const double *b,
                               const int32_t *m, const uint64_t *keep, const double *xc, const double *scale,
                               double *volume, double *area, int32_t *status);

/*
 * Containment of N points in P polytopes:  all_i( A_p[i,:].x - b_p[i] < abs_tol ).
 * Replaces: Polytope.contains (polytope/polytope.py:206-218), Region.contains (:732-746),
 *           is_inside (:1017-1029), __contains__ (:191-204, :723-730).
 * X[d][N]: column vectors exactly as the reference takes them.
 * mode 0 (Region.contains): out[N]    = OR over the P polytopes (all P*N tests evaluated)
 * mode 1 (per polytope)   : out[P][N] = Polytope.contains of each polytope
 */
int plp_contains(plp_ctx *ctx, int P, int m_max, int d, const double *A, const double *b, const int32_t *m,
                 int64_t N, const double *X, double abs_tol, int mode, uint8_t *out);
int plp_contains_dev(plp_ctx *ctx, void *stream, int P, int m_max, int d, const double *A, const double *b,
                     const int32_t *m, int64_t N, const double *X, double abs_tol, int mode, uint8_t *out);

/*
 * Point location: for each of N points the FIRST of P polytopes that contains it, and optionally how many do.
 * No counterpart in the reference, whose users loop `x in region` over a partition one point at a time.
 * In:  A[P][m_max][d], b[P][m_max], m[P] (NULL = m_max), X[d][N] and abs_tol exactly as plp_contains takes them.
 * Out: first[N] = min { p : all_{i < m[p]} (fl(A_p[i].x) - b_p[i]) < abs_tol }  or -1, the dot product in
 *      plp_contains' arithmetic (s = a0 x0; s = fma(a_k, x_k, s), k ascending): first[q] is the arg-max over p of
 *      plp_contains' mode-1 matrix wherever column q holds a 1;
 *      count[N] (NULL: not computed, and the search for a point stops at its first hit) = the number of such p.
 *      A polytope with m[p] = 0 contains every point (NaN points too); a point with a NaN coordinate is in no polytope
 *      that has a row.
 * grid == NULL: every polytope is tested against every point (wave-uniform rows, as plp_contains).
 * grid != NULL (a HOST pointer in both forms): a uniform grid over up to PLP_LOCATE_MAX_AXES coordinate axes culls the
 *      candidates.  Axis j of the grid is coordinate axis[j], cut into res[j] cells of width 1 / inv_h[j] from lo[j] on;
 *      cell_j(x) = (int) fmin(fmax(floor((x - lo[j]) * inv_h[j]), 0), res[j] - 1), NaN -> 0; the flat cell number is
 *      row-major over j.  G = prod res[j] <= PLP_LOCATE_MAX_CELLS.  cell_start[G + 1] and cell_items[cell_start[G]] are
 *      the lists plp_locate_grid_count / _fill build: cell c holds polytopes cell_items[cell_start[c] .. cell_start[c + 1]),
 *      ascending.  The answer equals the dense one provided every polytope is listed in the cell of every point it contains.
 * plp_locate_grid_count: a polytope is listed in the cells [cell_j(lb_j - pad'), cell_j(ub_j + pad')] of its box
 *      lb[P][d], ub[P][d] (pad' = pad * max(1, the box's largest finite |bound| on any axis); +-inf sides and NaN bounds span the axis; lb_j - pad' > ub_j + pad'
 *      on a gridded axis -- e.g. lb = +inf, ub = -inf -- lists it nowhere).  Writes the exclusive prefix sums of the list
 *      lengths to cell_start[G + 1] (saturating at 2^31 - 1) and the longest list's length to max_len[1].
 * plp_locate_grid_fill: with that cell_start, writes cell_items (cell_start[G] entries, every list sorted ascending, so
 *      the result is deterministic); cursor[G] is scratch.
 * Errors, as plp_contains: negative sizes, d < 1, a bad grid descriptor: PLP_EINVAL "bad sizes"; NULL first / X / lists:
 *      PLP_EINVAL "NULL pointer"; d > 16: PLP_EUNSUPPORTED.  N = 0 returns at once; P = 0 writes first = -1, count = 0.
 */
#define PLP_LOCATE_MAX_AXES 3
#define PLP_LOCATE_MAX_CELLS (1 << 18)
typedef struct plp_locate_grid {
    int32_t naxes;                      /* 1 .. PLP_LOCATE_MAX_AXES */
    int32_t axis[PLP_LOCATE_MAX_AXES];  /* distinct coordinate axes, each < d */
    int32_t res[PLP_LOCATE_MAX_AXES];   /* cells along each, >= 1 */
    int32_t reserved;
    double lo[PLP_LOCATE_MAX_AXES];     /* lower end of cell 0 */
    double inv_h[PLP_LOCATE_MAX_AXES];  /* 1 / cell width, >= 0 (0: one cell) */
} plp_locate_grid;
int plp_locate(plp_ctx *ctx, int P, int m_max, int d, const double *A, const double *b, const int32_t *m, int64_t N,
               const double *X, double abs_tol, const plp_locate_grid *grid, const int32_t *cell_start,
               const int32_t *cell_items, int32_t *first, int32_t *count);
int plp_locate_dev(plp_ctx *ctx, void *stream, int P, int m_max, int d, const double *A, const double *b,
                   const int32_t *m, int64_t N, const double *X, double abs_tol, const plp_locate_grid *grid,
                   const int32_t *cell_start, const int32_t *cell_items, int32_t *first, int32_t *count);
int plp_locate_grid_count(plp_ctx *ctx, int P, int d, const double *lb, const double *ub, double pad,
                          const plp_locate_grid *grid, int32_t *cell_start, int32_t *max_len);
int plp_locate_grid_count_dev(plp_ctx *ctx, void *stream, int P, int d, const double *lb, const double *ub, double pad,
                              const plp_locate_grid *grid, int32_t *cell_start, int32_t *max_len);
int plp_locate_grid_fill(plp_ctx *ctx, int P, int d, const double *lb, const double *ub, double pad,
                         const plp_locate_grid *grid, const int32_t *cell_start, int32_t *cursor, int32_t *cell_items);
int plp_locate_grid_fill_dev(plp_ctx *ctx, void *stream, int P, int d, const double *lb, const double *ub, double pad,
                             const plp_locate_grid *grid, const int32_t *cell_start, int32_t *cursor,
                             int32_t *cell_items);

/*
 * quickhull outside-set assignment and furthest point.
 * Replaces: distance() (polytope/quickhull.py:117-121), the assignment loops (:224-245,
 *           :311-336: a point goes to the FIRST facet with distance > abs_tol) and
 *           Facet.get_furthest (:87-102: first maximum wins).
 * X[N][d] (rows = points, as quickhull takes them), normals[F][d], offsets[F].
 * Out: facet_of_point[N] (-1 = inside every facet), dist[N] (0 when unassigned),
 *      argmax[F] (index of the furthest point assigned to facet f, -1 if none), maxd[F] (its
 *      distance; 0 if none).
 */
int plp_assign(plp_ctx *ctx, int64_t N, int d, const double *X, int F, const double *normals,
               const double *offsets, double abs_tol, int32_t *facet_of_point, double *dist,
               int64_t *argmax, double *maxd);
int plp_assign_dev(plp_ctx *ctx, void *stream, int64_t N, int d, const double *X, int F,
                   const double *normals, const double *offsets, double abs_tol, int32_t *facet_of_point,
                   double *dist, int64_t *argmax, double *maxd);

/*
 * quickhull main loop: outside sets kept on the device for the whole run.
 * Replaces: the per-iteration pooling of the visible facets' outside points and their
 *           re-assignment to the new facets (polytope/quickhull.py:273-283, :311-336), the initial
 *           assignment (:224-245) and Facet.get_furthest (:87-102).
 * A plp_hull holds the N points ([N][d] rows, uploaded once), one int32 owner per point (facet id;
 * -1 = not outside any facet) and the point's distance to its owner.  Facet ids are handed out by
 * the session in creation order; id 0 is the virtual facet that owns every point at creation.
 *
 * plp_hull_reassign: flag the n_dead facets dead_ids[] (the visible set) dead; every point they own
 *   goes to the FIRST of the n_new facets normals[n_new][d], offsets[n_new] (creation order) with
 *   n.p - offset > abs_tol, else to -1.  The new facets get ids *new_id0 .. *new_id0 + n_new - 1.
 *   Out (per new facet): count[] points received, argmax[] the point furthest from it (-1 if none;
 *   lowest point index among exactly equal distances), maxd[] that distance (0 if none).
 * plp_hull_drop: owner[idx[i]] = -1 (start-simplex members, the apex just taken from its facet).  The
 *   indices are copied before the call returns; the update itself is enqueued and ordered before the
 *   session's next call (reassign and read synchronise).
 * A call moves its small arrays through one pinned block: one H2D copy, the kernels, one D2H copy.
 * plp_hull_read: copy owner[N] / dist[N] to the host (either may be NULL).
 * The "_dev" form is stateless: device pointers X, owner, dist, dead[new_id0] (uint8 per facet id),
 * normals, offsets, argmax, maxd, count; it enqueues on `stream` and returns.
 */
typedef struct plp_hull plp_hull;
int plp_hull_create(plp_ctx *ctx, int64_t N, int d, const double *X, plp_hull **out);
int plp_hull_destroy(plp_hull *h);
int plp_hull_drop(plp_hull *h, int64_t n, const int64_t *idx);
int plp_hull_reassign(plp_hull *h, int n_dead, const int32_t *dead_ids, int n_new, const double *normals,
                      const double *offsets, double abs_tol, int32_t *new_id0, int64_t *argmax,
                      double *maxd, int64_t *count);
int plp_hull_read(plp_hull *h, int32_t *owner, double *dist);
int plp_hull_reassign_dev(plp_ctx *ctx, void *stream, int64_t N, int d, const double *X, int32_t *owner,
                          double *dist, const uint8_t *dead, int new_id0, int n_new, const double *normals,
                          const double *offsets, double abs_tol, int64_t *argmax, double *maxd,
                          int64_t *count);

/*
 * Adjacency of all pairs of n cells (one polytope each): adj[i][j] = 1 iff the two cells, both
 * inflated by abs_tol, have an intersection with Chebyshev radius > abs_tol/10.
 * Replaces: the O(n^2) loop of find_adjacent_regions (polytope/prop2partition.py:46-63) over
 *           is_adjacent(a, b, overlap=True) (polytope/polytope.py:1843-1866): one Chebyshev LP per
 *           pair on the stacked rows [A_i; A_j], [b_i + abs_tol; b_j + abs_tol].
 * A[n][m_max][d], b[n][m_max], m[n] or NULL; 2*m_max <= 64, d <= 16 (d >= 9: one pair per wavefront).  Out: adj[n][n] (symmetric,
 * ones on the diagonal).  The n(n-1)/2 pair LPs are formed on the device from the resident cells.
 */
int plp_adjacent_pairs(plp_ctx *ctx, int n, int m_max, int d, const double *A, const double *b,
                       const int32_t *m, double abs_tol, uint8_t *adj);
int plp_adjacent_pairs_dev(plp_ctx *ctx, void *stream, int n, int m_max, int d, const double *A,
                           const double *b, const int32_t *m, double abs_tol, uint8_t *adj);
/*
 * Overlap of all pairs of n cells: out[i][j] = 1 iff the stack of cells i and j (nothing inflated) has
 * Chebyshev radius > abs_tol, i.e. is_fulldim(cell_i.intersect(cell_j)); ones on the diagonal.
 * Replaces: the O(n^2) pair loop of Partition.are_disjoint (polytope/prop2partition.py:123-192).
 */
int plp_overlap_pairs(plp_ctx *ctx, int n, int m_max, int d, const double *A, const double *b,
                      const int32_t *m, double abs_tol, uint8_t *out);
int plp_overlap_pairs_dev(plp_ctx *ctx, void *stream, int n, int m_max, int d, const double *A,
                          const double *b, const int32_t *m, double abs_tol, uint8_t *out);
/*
 * Cross pairs of TWO lists of cells held in one table (the first n1 cells, then n2 cells; A[n1+n2][m_max][d] ...):
 * out[a * n2 + c] = 1 iff the stack [cell a of the first list; cell c of the second] has a Chebyshev radius > thresh
 * (status 0), else 0.  Replaces: the scan region_diff opens with, one Chebyshev LP per cell of the subtrahend
 * (polytope/polytope.py:2148-2158), repeated by mldivide for every member of the minuend (:1484-1496) and by
 * Partition.refines for every pair of elements (prop2partition.py:194-207) -- here all n1 * n2 LPs in one launch, the
 * stacked rows formed on the device from the resident table.  2 * m_max <= 64, d <= 16.
 */
int plp_overlap_cross(plp_ctx *ctx, int n1, int n2, int m_max, int d, const double *A, const double *b,
                      const int32_t *m, double thresh, uint8_t *out);
int plp_overlap_cross_dev(plp_ctx *ctx, void *stream, int n1, int n2, int m_max, int d, const double *A,
                          const double *b, const int32_t *m, double thresh, uint8_t *out);

/*
 * plp_adjacent_pairs for a slice of the pair space (one rank's shard when the O(n^2) loop is split across
 * GPUs): pairs pair_lo <= p < pair_hi in the order p = i (i - 1) / 2 + j, j < i; out[p - pair_lo].
 */
int plp_adjacent_pairs_range(plp_ctx *ctx, int n, int m_max, int d, const double *A, const double *b,
                             const int32_t *m, double abs_tol, int64_t pair_lo, int64_t pair_hi,
                             uint8_t *out);
int plp_adjacent_pairs_range_dev(plp_ctx *ctx, void *stream, int n, int m_max, int d, const double *A,
                                 const double *b, const int32_t *m, double abs_tol, int64_t pair_lo,
                                 int64_t pair_hi, uint8_t *out);

/*
 * The pair verdicts of a LIST of pairs: out[t] is the byte the calls above give the pair (pairs[t][0], pairs[t][1]) of the
 * n cells -- 1 iff the stack of the two cells, every b raised by `inflate`, has a Chebyshev radius > thresh (adjacency:
 * inflate = abs_tol, thresh = abs_tol / 10; overlap: inflate = 0, thresh = abs_tol).  The same engines (picked by K as the
 * dense calls pick by their pair count) and the same careful pass, so the bytes are equal, pair for pair.  A pair may be
 * listed more than once and in either order.  pairs[K][2] int32.  2 * m_max <= 64, d <= 16.
 * A pair with an index outside [0, n) or with two equal indices: the host-pointer call returns PLP_EINVAL before anything
 * runs; the device-pointer call, which cannot read the list, writes PLP_PAIR_BAD for that pair and reads nothing for it.
 */
#define PLP_PAIR_BAD 255
int plp_pair_list(plp_ctx *ctx, int n, int m_max, int d, const double *A, const double *b, const int32_t *m,
                  double inflate, double thresh, int64_t K, const int32_t *pairs, uint8_t *out);
int plp_pair_list_dev(plp_ctx *ctx, void *stream, int n, int m_max, int d, const double *A, const double *b,
                      const int32_t *m, double inflate, double thresh, int64_t K, const int32_t *pairs, uint8_t *out);

/*
 * Closest points and Euclidean distances of a LIST of cell pairs:  min |x - y|_2  s.t.  A_i x <= b_i,  A_j y <= b_j  for
 * pair t = (pairs[t][0], pairs[t][1]) = (i, j) of the n cells -- a GJK iteration per pair on the Minkowski difference, its
 * support points from the support LP of plp_support_batch, two lanes per pair (csrc/plp_pair_dist.hpp).
 * In:  A[n][m_max][d], b[n][m_max], m[n] (NULL = m_max);  xc[n][d]: a STRICTLY interior point per cell, as for
 *      plp_support_batch;  pairs[K][2] int32, a pair may be listed more than once and in either order.
 * Out: dist[K] = |x - y|_2;  lb[K] (NULL ok): the lower bound -h_i(-u) - h_j(u), u = (x - y) / dist, the iteration ended with,
 *      held to [0, dist];  x[K][d], y[K][d] (NULL ok): the closest points, x in cell i and y in cell j;  status[K]:
 *        0  settled.  With E = max(1, |x|_inf, |y|_inf):  dist - max(lb, 0) <= 1e-10 E  or  dist <= 1e-10 E  (the cells meet:
 *           lb = 0), and x, y are inside every row of their cells to 1e-10 E on unit-scaled slack.  With the bounds of the
 *           two support values that gives  -2e-10 E <= dist - dist* <= 5e-10 E'  (E' the extent of the last support points;
 *           the derivation is in csrc/plp_pair_dist.hpp);
 *        1  NOT SETTLED HERE (dist = lb = x = y = NaN): a support LP was handed back, a centre is not strictly inside its
 *           cell or not finite, a row is not finite, the round cap (16), or a stall.  The caller settles these
 *           (polytope_amd.batch: distance_pairs(resolve=True));
 *        3  a support LP came back unbounded: a cell is unbounded in a direction the iteration asked for, which includes a
 *           cell without rows.  NaN outputs; not settled by this call;
 *        PLP_PAIR_BAD (255)  an index outside [0, n) or i == j, device-pointer form only: NaN outputs, and nothing of the table
 *           is read for the pair.  The host-pointer form returns PLP_EINVAL for such a list before anything runs.
 * d <= 4, m_max <= 64 and K <= 2^31 - 1, else PLP_EUNSUPPORTED.  K = 0 or n = 0: returns PLP_OK, nothing runs.
 * The host-pointer form checks A and b for inf / nan when the context asks for it (plp_ctx_set_check_finite).  The call
 * runs on the caller's stream and needs no scratch.
 */
int plp_pair_dist(plp_ctx *ctx, int n, int m_max, int d, const double *A, const double *b, const int32_t *m,
                  const double *xc, int64_t K, const int32_t *pairs, double *dist, double *lb, double *x, double *y,
                  int32_t *status);
int plp_pair_dist_dev(plp_ctx *ctx, void *stream, int n, int m_max, int d, const double *A, const double *b,
                      const int32_t *m, const double *xc, int64_t K, const int32_t *pairs, double *dist, double *lb,
                      double *x, double *y, int32_t *status);

/*
 * The broad phase in front of plp_pair_list: the pairs of cells whose outer boxes meet.  Cell p has the box lb[p][d],
 * ub[p][d], padded to L_p = lb_p - pad', U_p = ub_p + pad' with pad' = pad * max(1, the box's largest finite |bound|); NaN
 * bounds and infinite sides span their axis (as plp_locate_grid_count).  (i, j) is a CANDIDATE iff
 * max(L_i[k], L_j[k]) <= min(U_i[k], U_j[k]) on all d axes.  If every finite side bounds the cell {A x <= b + inflate}, a
 * pair that is no candidate has verdict 0 in plp_pair_list: a ball of radius r > thresh >= 0 in both cells lies in both boxes.
 * n1 == 0: the pairs (i, j) with j < i.  n1 > 0, the cross form: the table holds n1 cells and then n - n1, and the pairs are
 *      (a, c) with a < n1 <= c.
 * grid == NULL: every partner is box-tested.  grid != NULL (a HOST pointer in both forms) with cell_start / cell_items, the
 *      lists plp_locate_grid_count / _fill build from the SAME lb, ub and pad: partners are met through the lists, each
 *      pair in one canonical grid cell.  The set of candidates is the same, integer for integer.
 * plp_box_pairs_count: per_cell[n + 1] (int64), the exclusive prefix sums of the cells' numbers of partners; per_cell[n] = K.
 * plp_box_pairs_fill: with that per_cell, the pairs of the cells cell_lo <= i < cell_hi into
 *      pairs[per_cell[cell_hi] - per_cell[cell_lo]][2] (int32): (i, j), cell i's partners ascending, so the list is sorted
 *      by (i, j) and deterministic.  Count and fill evaluate one predicate.
 * Errors: negative sizes, d < 1, n1 > n, pad < 0, a bad grid descriptor or cell range: PLP_EINVAL "bad sizes"; NULL
 *      arrays: PLP_EINVAL "NULL pointer"; d > 16: PLP_EUNSUPPORTED.
 */
int plp_box_pairs_count(plp_ctx *ctx, int n, int d, const double *lb, const double *ub, double pad,
                        const plp_locate_grid *grid, const int32_t *cell_start, const int32_t *cell_items, int n1,
                        int64_t *per_cell);
int plp_box_pairs_count_dev(plp_ctx *ctx, void *stream, int n, int d, const double *lb, const double *ub, double pad,
                            const plp_locate_grid *grid, const int32_t *cell_start, const int32_t *cell_items, int n1,
                            int64_t *per_cell);
int plp_box_pairs_fill(plp_ctx *ctx, int n, int d, const double *lb, const double *ub, double pad,
                       const plp_locate_grid *grid, const int32_t *cell_start, const int32_t *cell_items, int n1,
                       const int64_t *per_cell, int cell_lo, int cell_hi, int32_t *pairs);
int plp_box_pairs_fill_dev(plp_ctx *ctx, void *stream, int n, int d, const double *lb, const double *ub, double pad,
                           const plp_locate_grid *grid, const int32_t *cell_start, const int32_t *cell_items, int n1,
                           const int64_t *per_cell, int cell_lo, int cell_hi, int32_t *pairs);

/*
 * The STACKS of a list of cell pairs: for pair t = (pairs[t][0], pairs[t][1]) = (i, j) of the n cells, what
 * Polytope(np.vstack([A_i, A_j]), np.hstack([b_i, b_j])) holds (polytope.py:272-275, constructor :130-138): the m_i rows
 * of cell i, then the m_j rows of cell j, each scaled by the reciprocal of its norm (sqrt of numpy's add.reduce of the
 * squares), rows of norm <= 1e-10 dropped and the rows behind them moved up.  W = 2 * m_max row slots per stack:
 * A_s[K][W][d], b_s[K][W], m_s[K] = rows that stay; rows from m_s[t] on are zero.  A packed table like any other: it goes
 * into plp_cheby_batch, plp_reduce_batch, plp_volume_hits, ... as it is.  2 * m_max <= 64, d <= 16 (else
 * PLP_EUNSUPPORTED).  A pair may be listed more than once and in either order (the order decides the row order).
 * A pair with an index outside [0, n) or with two equal indices: the host-pointer call returns PLP_EINVAL before anything
 * runs; the device-pointer call reads nothing of the table for it and writes m_s = 0 and zero rows.
 */
int plp_pair_stacks(plp_ctx *ctx, int n, int m_max, int d, const double *A, const double *b, const int32_t *m, int64_t K,
                    const int32_t *pairs, double *A_s, double *b_s, int32_t *m_s);
int plp_pair_stacks_dev(plp_ctx *ctx, void *stream, int n, int m_max, int d, const double *A, const double *b,
                        const int32_t *m, int64_t K, const int32_t *pairs, double *A_s, double *b_s, int32_t *m_s);

/*
 * The INTERSECTIONS of a list of cell pairs: per pair exactly what plp_reduce_batch returns for the stack above --
 * keep[K] (bit s = stack row s; where ms[t] == m_i + m_j the first m_i bits are cell i's rows), flags[K], r[K], xc[K][d],
 * nlp[K] -- and ms[K], the rows of the stack.  With A_out != NULL also the result's rows as plp_fm_emit(col = -1) forms
 * them from the reduce's keep and flags: A_out[K][mo_max][d], b_out[K][mo_max], m_out[K] (-1: more than mo_max rows; 0 under
 * PLP_RF_EMPTY / PLP_RF_LPFAIL / PLP_RF_F1OPEN), a packed table again.
 * The list is worked off in chunks of at most `chunk` pairs (chunk <= 0: the library's default, 32 MiB of stacks): stack ->
 * fused reduce -> emission, the stacks of one chunk in per-stream scratch; the stacks of the whole list are never resident.
 * Bad pairs as above; the device-pointer call writes keep = 0, flags = PLP_RF_EMPTY | PLP_RF_BADPAIR, r = 0, xc = NaN,
 * nlp = 0, ms = 0, m_out = 0 for such a pair and the other pairs of the list are not affected.
 */
#define PLP_RF_BADPAIR 64
/* the chunk plp_intersect_pairs uses for chunk <= 0 at this table shape (pairs; needs no context) */
int64_t plp_pair_chunk_default(int m_max, int d);
int plp_intersect_pairs(plp_ctx *ctx, int n, int m_max, int d, const double *A, const double *b, const int32_t *m,
                        double abs_tol, int64_t K, const int32_t *pairs, int64_t chunk, uint64_t *keep, int32_t *flags,
                        double *r, double *xc, int32_t *nlp, int32_t *ms, int mo_max, double *A_out, double *b_out,
                        int32_t *m_out);
int plp_intersect_pairs_dev(plp_ctx *ctx, void *stream, int n, int m_max, int d, const double *A, const double *b,
                            const int32_t *m, double abs_tol, int64_t K, const int32_t *pairs, int64_t chunk,
                            uint64_t *keep, int32_t *flags, double *r, double *xc, int32_t *nlp, int32_t *ms, int mo_max,
                            double *A_out, double *b_out, int32_t *m_out);

/*
 * Quickhull's main loop (polytope/quickhull.py:224-345) as native host code over a plp_hull session: facet graph,
 * visibility search, horizon, new facets and their links on the host, every pass over the points one plp_hull_reassign.
 * X0[N][d]: the points translated so that the start simplex' centroid is the origin (:188-192); simplex[d + 1]: the
 * indices of the start simplex (chosen by the caller, who owns the random number stream, :165-185).
 * lapack_dgesv: optional pointer to LAPACK's dgesv (Fortran calling convention) for the facet hyperplanes (:66-85);
 * with the one numpy.linalg.solve runs, the rows come out bit-identical to the reference's; NULL = built-in LU.
 * Result: the hull's facets in the reference's order: normals[n][d] (unit, outward), offsets[n] (translated
 * coordinates: n.x = offset), verts[n][d] point indices.  PLP_EINVAL + plp_quickhull_last_error() for a singular
 * hyperplane system / degenerate neighbouring facets (where the reference raises).
 */
typedef struct plp_qh_result plp_qh_result;
int plp_quickhull_run(plp_ctx *ctx, int64_t N, int d, const double *X0, const int64_t *simplex, double abs_tol,
                      void *lapack_dgesv, plp_qh_result **out);
int plp_qh_result_sizes(const plp_qh_result *r, int64_t *n_facets, int64_t *iterations, int64_t *facets_made);
int plp_qh_result_copy(const plp_qh_result *r, double *normals, double *offsets, int64_t *verts);
int plp_qh_result_free(plp_qh_result *r);
const char *plp_quickhull_last_error(void);

/*
 * The search of region_diff: poly minus the union of N cells (polytope/polytope.py:2201-2281), run by the library.
 * The caller has done the reference's preparation (:2144-2199): cells sorted by the Chebyshev radius of their stack
 * with poly, mi[j] >= 1 new constraints per cell, and the table  A[m + 2M][d], b[m + 2M]  (M = sum mi) = poly's m rows,
 * the cells' new rows in that order, and the negations of those M rows -- each row already scaled to unit length as
 * Polytope.__init__ does (:130-138), because every LP of the search is the Chebyshev ball (:1283-1288) of
 * Polytope(A[rows], b[rows]) for some row list.  The table is uploaded once; the library walks the reference's search
 * (same visiting order, same tests "R > abs_tol", including its index arithmetic on INDICES / counter) and solves the
 * LPs in batches that are described by row-index lists only and gathered on the device; each batch holds what the
 * search needs now plus what it will need next if the current node is not empty (its scan and the first child of
 * every cell), so there is one launch and one synchronisation per visited node instead of one per LP.
 * Result: the pieces in the reference's order, as row lists: kind[k] = 0 -> Polytope(A[rows], b[rows]) as is (:2229),
 * 1 -> reduce() of it (:2276).  PLP_EINVAL with "row index out of range" where the reference raises IndexError.
 */
typedef struct plp_rdiff_result plp_rdiff_result;
int plp_region_diff_search(plp_ctx *ctx, int d, int m, int N, const int32_t *mi, const double *A, const double *b,
                           double abs_tol, plp_rdiff_result **out);
int plp_rdiff_result_sizes(const plp_rdiff_result *r, int64_t *n_leaves, int64_t *n_rows, int64_t *n_lps,
                           int64_t *n_batches);
/* kind[n_leaves], off[n_leaves + 1], rows[n_rows]: piece k holds rows[off[k] .. off[k+1]) */
int plp_rdiff_result_copy(const plp_rdiff_result *r, int32_t *kind, int32_t *off, int32_t *rows);
int plp_rdiff_result_free(plp_rdiff_result *r);

/*
 * B set differences in one launch: problem p is the minuend A[p] (m[p] rows) minus the cells cell_idx[cell_off[p] ..
 * cell_off[p + 1]), in that order, of the shared packed cell table CA[Nc][mc_max][d], Cb[Nc][mc_max], mc[Nc] (NULL =
 * mc_max).  All rows are unit length already (Polytope.__init__, :130-138) and the cells are sorted as region_diff sorts
 * them (:2153-2157).  One wavefront builds the table of its problem (region_diff :2166-2183: a cell row is new when
 * sum_k |row_c[k] - row_p[k]| over (a, b) is >= abs_tol for every minuend row p) and runs the whole search of
 * plp_region_diff_search on it, one Chebyshev LP per radius it reads; no host round trip.
 * Caps per problem: d <= 4, m <= 64, at most 64 cells of at most 64 rows, m + 2M <= 256 table rows, lists of <= 64 rows.
 * Out, per problem: the pieces in the reference's order as lists of LOCAL table rows (0 .. m - 1 the minuend's, m + k new
 *      row k, m + M + k its negation): kind[B][p_max] (0 = as is, 1 = to be reduce()d), off[B][p_max + 1],
 *      rows[B][r_max]; count[B] / nrows[B] pieces and rows produced; nlp[B] LPs run; mi[B][n_max] new rows per cell;
 *      src[B][M_max] the cell-table row c * mc_max + r of new row k; status[B]:
 *        PLP_RD_OK;
 *        PLP_RD_OVERFLOW     more than p_max pieces or r_max rows: count / nrows hold what is needed, what fits is written;
 *        PLP_RD_COVERED      a listed cell has no new row: the difference is empty, count 0;
 *        PLP_RD_LONG         a list of more than 64 rows;
 *        PLP_RD_BUDGET       max_lps LPs did not finish the search;
 *        PLP_RD_INDEX        the reference raises IndexError here (its index arithmetic on INDICES left the table);
 *        PLP_RD_UNSUPPORTED  a cap on m / the cells / M, or a cell index outside the table: nothing is run.
 * cell_off[B + 1] must be non-decreasing from cell_off[0] >= 0, and cell_idx must hold cell_off[B] entries: the host-pointer
 * form returns PLP_EINVAL otherwise; the _dev form cannot see the arrays, ends a problem whose own two entries are negative
 * or decreasing as PLP_RD_UNSUPPORTED, and relies on the caller for the length of cell_idx.
 * B = 0: returns PLP_OK, nothing runs.  d > 4: PLP_EUNSUPPORTED.
 */
#define PLP_RD_OK 0
#define PLP_RD_OVERFLOW 1
#define PLP_RD_COVERED 2
#define PLP_RD_LONG 3
#define PLP_RD_BUDGET 4
#define PLP_RD_INDEX 5
#define PLP_RD_UNSUPPORTED 6
int plp_region_diff_batch(plp_ctx *ctx, int64_t B, int m_max, int d, const double *A, const double *b, const int32_t *m,
                          int64_t Nc, int mc_max, const double *CA, const double *Cb, const int32_t *mc,
                          const int32_t *cell_off, const int32_t *cell_idx, double abs_tol, int max_lps, int p_max, int r_max,
                          int n_max, int M_max, int32_t *kind, int32_t *off, int32_t *rows, int32_t *count, int32_t *nrows,
                          int32_t *nlp, int32_t *status, int32_t *mi, int32_t *src);
int plp_region_diff_batch_dev(plp_ctx *ctx, void *stream, int64_t B, int m_max, int d, const double *A, const double *b,
                              const int32_t *m, int64_t Nc, int mc_max, const double *CA, const double *Cb,
                              const int32_t *mc, const int32_t *cell_off, const int32_t *cell_idx, double abs_tol,
                              int max_lps, int p_max, int r_max, int n_max, int M_max, int32_t *kind, int32_t *off,
                              int32_t *rows, int32_t *count, int32_t *nrows, int32_t *nlp, int32_t *status, int32_t *mi,
                              int32_t *src);

/*
 * The facet tests of envelope() (polytope.py envelope, ref :1414-1464) for B regions in one launch.  The members of all
 * regions are one packed table A[C][mc_max][d], b[C][mc_max], mc[C] (NULL = mc_max) of unit rows; region p lists the
 * members mem_idx[reg_off[p] .. reg_off[p + 1]) (mem_idx NULL: list entry w is member w), L = the length of mem_idx.  Two
 * regions, or two entries of one region, may list the same member.  One wavefront takes one list entry w -- member
 * i = mem_idx[w] of its region -- and tests every row ii of i against every OTHER entry j of the same list: row ii is
 * crossed once the Chebyshev radius R of [rows of j; -a_ii x <= -b_ii] exceeds abs_tol, and outer otherwise.  Rows that are
 * crossed already are not tested again (the verdict is an OR: the order changes the LP count only).
 * A test with R NaN or abs_tol / 2 < R < 2 * abs_tol has no verdict: it neither crosses nor clears its row.
 * Caps: d <= 8, every listed member 1 .. 63 rows; no cap on the members of a region.
 * Out, per list entry: outer[L] (bit ii set = row ii of the member is outer), nlp[L] LPs run, status[L]:
 *        PLP_ENV_OK;
 *        PLP_ENV_OPEN         a row is not crossed and one of its tests had no verdict: outer holds it as outer;
 *        PLP_ENV_UNSUPPORTED  a listed member with no row or more than 63, a listed index outside the table, or no pair
 *                             reg_off[p] <= w < reg_off[p + 1] <= L around the entry (the region of w is found by bisection:
 *                             reg_off starts above w, decreases in front of it, or ends beyond L): nothing is run, outer 0.
 * Neither form reads mem_idx beyond L or the table beyond C members, whatever reg_off and mem_idx hold.
 * B = 0 or L = 0: returns PLP_OK, nothing runs.  d > 8: PLP_EUNSUPPORTED.
 * The _dev form enqueues on `stream` and uses no scratch of the context.
 */
#define PLP_ENV_OK 0
#define PLP_ENV_OPEN 1
#define PLP_ENV_UNSUPPORTED 2
int plp_envelope_batch(plp_ctx *ctx, int64_t C, int mc_max, int d, const double *A, const double *b, const int32_t *mc,
                       int64_t B, const int32_t *reg_off, int64_t L, const int32_t *mem_idx, double abs_tol, uint64_t *outer,
                       int32_t *status, int32_t *nlp);
int plp_envelope_batch_dev(plp_ctx *ctx, void *stream, int64_t C, int mc_max, int d, const double *A, const double *b,
                           const int32_t *mc, int64_t B, const int32_t *reg_off, int64_t L, const int32_t *mem_idx,
                           double abs_tol, uint64_t *outer, int32_t *status, int32_t *nlp);

/*
 * The projection of B polytopes {A x <= b} in R^d onto k of their coordinates by the iterative hull (polytope.py
 * projection_iterhull, ref :1955-2100) in one launch: one polytope per wavefront, its rows read once, every LP and every
 * hull rebuild inside the kernel (polytope_amd/csrc/plp_projhull.hpp holds the rule as host-compilable code).
 * In: A[B][m_max][d], b[B][m_max], m[B] (NULL = m_max; only rows below m[p] are read); keep[k]: the kept coordinates,
 * 0-based and increasing -- k integers in HOST memory in both forms; xc[B][d]: a strictly interior point of every polytope
 * (the Chebyshev centre).  The rule, per polytope:
 *   box     the 2k LPs max +x_j, max -x_j over the kept j, in that order; an unbounded one ends with PLP_PH_UNBOUNDED.
 *           Their projected points start the point list V and fix the frame: the centre c and half-extent s of the box.
 *           Every tolerance below is absolute on (p - c) / s.
 *   points  a new point within 1e-9 (max-norm) of one held is dropped; a 65th point: PLP_PH_OVERFLOW_POINTS.
 *   rank    while V has fewer than k + 1 points or is flat: the LPs +nu and -nu for a unit nu orthogonal to the span of V
 *           (Gram-Schmidt, largest residual first), the further point joins V; none further than 1e-8: PLP_PH_FLAT.
 *   rounds  the facets of V by the rule of plp_hull_batch.  A facet equal to one confirmed in an earlier round stays
 *           confirmed; for every other, in list order, the LP max nu . x: a value within 1e-8 of the facet's offset
 *           confirms it, otherwise the LP's point joins V.  A round that adds no point ends with the facet list as the
 *           answer; otherwise the facets are enumerated again.
 *   LPs     a point that violates a row by more than 1e-9 max(1, |b - A xc|_max), or an LP without a verdict:
 *           PLP_PH_LPFAIL; at most max_lps LPs: PLP_PH_BUDGET.
 * Out: Ao[B][f_max][k] (unit normals), bo[B][f_max], on[B][f_max] (bit i: point i of V lies on the facet), count[B] --
 * the rows of the projection in the caller's coordinates, NaN / 0 beyond count, written for PLP_PH_OK only (count = 0
 * otherwise); V[B][64][k], nv[B]: the points, NaN beyond nv; X[B][64][d] or NULL: a point of the polytope above every
 * entry of V; vmask[B]: bit i set when point i lies on at least k of the rows -- advisory: a near-duplicate tilted row
 * can set the bit of a point inside an edge; nlp[B]; status[B]:
 *        PLP_PH_OK, PLP_PH_UNBOUNDED, PLP_PH_FLAT, PLP_PH_OVERFLOW_POINTS, PLP_PH_OVERFLOW_FACETS (more than f_max facets),
 *        PLP_PH_BUDGET, PLP_PH_LPFAIL, PLP_PH_NOCENTRE (no row, an entry that is not finite, or b_i - a_i . xc <= 0 for a
 *        row: nothing was run).
 * Caps: 1 <= k <= 3, k <= d <= 16, m_max <= 64, 1 <= f_max <= 128 (the upper-bound theorem for 64 points in R^3 gives
 * 124), keep increasing and below d, B < 2^31: PLP_EUNSUPPORTED beyond.  B = 0: returns PLP_OK, nothing runs.
 * The _dev form enqueues on `stream` and uses no scratch of the context.
 */
#define PLP_PH_OK 0
#define PLP_PH_UNBOUNDED 1
#define PLP_PH_FLAT 2
#define PLP_PH_OVERFLOW_POINTS 3
#define PLP_PH_OVERFLOW_FACETS 4
#define PLP_PH_BUDGET 5
#define PLP_PH_LPFAIL 6
#define PLP_PH_NOCENTRE 7
#define PLP_PH_MAX_POINTS 64
int plp_project_hull_batch(plp_ctx *ctx, int64_t B, int m_max, int d, int k, const double *A, const double *b,
                           const int32_t *m, const int32_t *keep, const double *xc, int f_max, int max_lps, double *Ao,
                           double *bo, uint64_t *on, int32_t *count, double *V, int32_t *nv, double *X, uint64_t *vmask,
                           int32_t *nlp, int32_t *status);
int plp_project_hull_batch_dev(plp_ctx *ctx, void *stream, int64_t B, int m_max, int d, int k, const double *A,
                               const double *b, const int32_t *m, const int32_t *keep, const double *xc, int f_max,
                               int max_lps, double *Ao, double *bo, uint64_t *on, int32_t *count, double *V, int32_t *nv,
                               double *X, uint64_t *vmask, int32_t *nlp, int32_t *status);

/* cross-lane primitive self-test (group size 8/16/32/64); host out_d[128], out_u[128] */
int plp_selftest(plp_ctx *ctx, int group_size, double *out_d, uint32_t *out_u);

#ifdef __cplusplus
}
#endif
#endif /* PLP_H */
