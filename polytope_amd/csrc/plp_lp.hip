// plp_lp.hip -- the stand-alone LP family: the one-row-per-lane kernels and the launchers of the five calls (gfx950).
//
//   lp_kernel<N>    : B independent LPs  min c'x s.t. Gx<=h, x free   (solvers.py:76-106,149-158)
//   cheby_kernel<D> : B Chebyshev-ball LPs (form F1, polytope.py:1283-1288):
//                     c = -e_{d+1}, G = [A | sqrt(sum(A*A,1))], h = b
//
// One LP per lane group (GS lanes, GS >= rows), 64/GS LPs per wavefront, 256-thread workgroups, grid-stride over the
// batch.  These are the kernels of the batches no faster engine takes and of the retry pass behind lp_r_kernel; which
// engine a batch gets is plp_lp_plan.hpp's, and launch_lp_phase / launch_cheby / launch_bbox / launch_adjacent below
// carry its plan out.
#include "plp_lp_launch.hpp"
#include "plp_simplex.hpp"

namespace plp {

template <int N>
__global__ __launch_bounds__(BLOCK) void lp_kernel(long long B, int m_max, int gs,
                                                   const double* __restrict__ c,
                                                   const double* __restrict__ G,
                                                   const double* __restrict__ h,
                                                   const int* __restrict__ mrows,
                                                   double* __restrict__ x, double* __restrict__ fun,
                                                   int* __restrict__ status, int* __restrict__ iters,
                                                   int retry_only) {
    constexpr int NC = N + 1;  // + phase-1 artificial
    const Grp g(gs);
    const int gpb = BLOCK / gs;
    const int gib = threadIdx.x / gs;
    if (retry_only) {  // normally nothing was handed over: one round trip of status loads, then leave
        bool any = false;
        for (long long base = (long long)blockIdx.x * gpb; base < B; base += (long long)gridDim.x * gpb)
            any = any | ((base + gib < B) && status[base + gib] == ST_RETRY);
        if (!__syncthreads_or(any)) return;
    }
    for (long long base = (long long)blockIdx.x * gpb; base < B; base += (long long)gridDim.x * gpb) {
        const long long lp = base + gib;
        bool valid = lp < B;
        // second pass after lp_r_kernel: only the LPs it handed over (status ST_RETRY: phase 1 or Bland needed)
        if (retry_only) {
            valid = valid && status[lp] == ST_RETRY;
            if (!__any(valid)) continue;
        }
        const int m = valid ? (mrows ? mrows[lp] : m_max) : 0;
        const int i = g.gl;
        const bool has_row = valid && i < m;
        Simplex<NC, true> S;
        S.reset(N, m, i);
        double cc[N];
        bool finite = true;
#pragma unroll
        for (int j = 0; j < N; ++j) {
            cc[j] = valid ? c[lp * N + j] : 0.0;
            finite = finite && isfinite(cc[j]);
        }
        bool zero = true;
        double hi = 0.0;
        if (has_row) {
            const double* Gr = G + (lp * m_max + i) * N;
#pragma unroll
            for (int j = 0; j < N; ++j) {
                S.T[j] = Gr[j];
                zero = zero && (S.T[j] == 0.0);
                finite = finite && isfinite(S.T[j]);
            }
            hi = h[lp * m_max + i];
            finite = finite && isfinite(hi);
        }
        S.beta = hi;
        S.rowact = has_row && !zero;
        const bool infeasible0 = grp_ballot(has_row && zero && hi < -TOL_FEAS, g) != 0;  // 0 <= h_i < 0
        if (has_row && zero) S.beta = 0.0;
        const bool bad = grp_ballot(!finite, g) != 0 || m > gs;
        const bool need_p1 = grp_ballot(S.rowact && hi < 0.0, g) != 0;
        S.set_col(N, ID_T);
        if (need_p1) {
            S.T[N] = S.rowact ? -1.0 : 0.0;
            S.cost[N] = 1.0;
#pragma unroll
            for (int j = 0; j < N; ++j) S.cost2[j] = cc[j];
            S.mode = M_INIT;
            S.init_col = N;
            S.init_q = S.beta;
            S.init_elig = S.rowact;
            S.mode_after_init = M_P1;
        } else {
#pragma unroll
            for (int j = 0; j < N; ++j) S.cost[j] = cc[j];
            S.dead = 1u << N;
            S.mode = M_P2;
        }
        if (!valid) { S.mode = M_DONE; S.status = ST_NUM; }
        else if (bad) { S.mode = M_DONE; S.status = ST_NUM; }
        else if (infeasible0) { S.mode = M_DONE; S.status = ST_INFEAS; }

        S.run(g);

        // gather x: variable j sits in the row whose basic id is j (0 when nonbasic)
        const bool ok = S.status == ST_OPT;
        const double mine = S.x_value();
        const bool holds = S.holds_x();
        double f = 0.0;
        const double qnan = __longlong_as_double(0x7ff8000000000000ll);
#pragma unroll
        for (int j = 0; j < N; ++j) {
            const uint64_t ob = grp_ballot(holds && S.rowvar == j, g);
            const double v = bcast(mine, g.gbase + (ob ? __ffsll((long long)ob) - 1 : 0));
            const double xj = ob ? v : 0.0;
            f = fma(cc[j], xj, f);
            if (valid && g.gl == 0) x[lp * N + j] = ok ? xj : qnan;
        }
        if (valid && g.gl == 0) {
            fun[lp] = ok ? f : qnan;
            status[lp] = S.status;
            if (iters) iters[lp] = S.iters;
        }
    }
}

template <int D>
__global__ __launch_bounds__(BLOCK) void cheby_kernel(long long B, int m_max, int gs,
                                                      const double* __restrict__ A,
                                                      const double* __restrict__ b,
                                                      const int* __restrict__ mrows,
                                                      double* __restrict__ r, double* __restrict__ xc,
                                                      int* __restrict__ status) {
    constexpr int NC = D + 1;
    const Grp g(gs);
    const int gpb = BLOCK / gs;
    const int gib = threadIdx.x / gs;
    for (long long base = (long long)blockIdx.x * gpb; base < B; base += (long long)gridDim.x * gpb) {
        const long long p = base + gib;
        const bool valid = p < B;
        const int m = valid ? (mrows ? mrows[p] : m_max) : 0;
        const int i = g.gl;
        const bool has_row = valid && i < m;
        double a[D], bi = 0.0;
#pragma unroll
        for (int k = 0; k < D; ++k) a[k] = 0.0;
        if (has_row) {
            const double* Ar = A + (p * m_max + i) * D;
#pragma unroll
            for (int k = 0; k < D; ++k) a[k] = Ar[k];
            bi = b[p * m_max + i];
        }
        double x[NC], inv_nrm;
        const int st = cheby_lp<D>(g, valid, has_row, m, gs, a, bi, x, inv_nrm);
        const bool ok = st == ST_OPT;
        const double qnan = __longlong_as_double(0x7ff8000000000000ll);
        if (valid && g.gl == 0) {
#pragma unroll
            for (int j = 0; j < D; ++j) xc[p * D + j] = ok ? x[j] : qnan;
            r[p] = ok ? x[D] : qnan;
        }
        if (valid && g.gl == 0) status[p] = st;
    }
}

// one launch of lp_kernel<n> as planned; retry_only: the second pass over the LPs left ST_RETRY
static int launch_lp_general(int n, const LpLaunch& L, const LpArgs& a, int retry_only, hipStream_t st) {
    return for_dim<1, MAX_D + 1>(n, [&](auto K) {
        hipLaunchKernelGGL(lp_kernel<decltype(K)::value>, dim3((unsigned)L.grid), dim3(L.block), L.lds, st, a.B, a.m_max, L.gs,
                           a.c, a.G, a.h, a.mrows, a.x, a.fun, a.status, a.iters, retry_only);
    });
}

// phase 0: everything, back to back.  phase 1: the fast kernels only -- *more = 1 when LPs they hand over (status ST_RETRY)
// may exist and the caller has to look; phase 2: the general kernel over exactly those.  The synchronous host entry point
// uses the phases for small batches: the normally idle general pass is a launch saved.
int launch_lp_phase(long long B, int m_max, int n, const double* c, const double* G, const double* h, const int* mrows,
                    double* x, double* fun, int* status, int* iters, hipStream_t st, int phase, int* more) {
    if (more) *more = 0;
    const LpPlan p = plan_lp(B, m_max, n, lp_env());
    const LpArgs a{B, m_max, c, G, h, mrows, x, fun, status, iters};
    if (phase == 2)   // (the LDS and the one-LP-per-wavefront engines hand nothing over)
        return (p.first.engine == LE_LDS || p.first.engine == LE_WIDE) ? 0 : p.first.engine == LE_NONE ? 2
                                                                            : launch_lp_general(n, p.retry, a, 1, st);
    switch (p.first.engine) {
        case LE_LDS: return launch_lp_lds(n, p.first, a, st);
        case LE_WIDE: return launch_lp_w(n, p.first, a, st);
        case LE_GENERAL: return launch_lp_general(n, p.first, a, 0, st);
        case LE_GROUP:
            if (launch_lp_r(n, p.first, p.p1 ? &p.p1_launch : nullptr, a, st)) return 2;
            if (phase == 1) {
                if (more) *more = 1;
                return 0;
            }
            return launch_lp_general(n, p.retry, a, 1, st);
        default: return 2;
    }
}

int launch_lp(long long B, int m_max, int n, const double* c, const double* G, const double* h, const int* mrows,
              double* x, double* fun, int* status, int* iters, hipStream_t st) {
    return launch_lp_phase(B, m_max, n, c, G, h, mrows, x, fun, status, iters, st, 0, nullptr);
}

int launch_cheby(long long B, int m_max, int d, const double* A, const double* b, const int* mrows, double* r,
                 double* xc, int* status, hipStream_t st) {
    const ChebyPlan p = plan_cheby(B, m_max, d, lp_env());
    const LpLaunch& L = p.first;
    const ChebyArgs a{B, m_max, A, b, mrows, r, xc, status};
    switch (L.engine) {
        case LE_LDS: return launch_cheby_lds(d, L, a, st);
        case LE_WIDE: return launch_cheby_w(d, L, a, st);
        case LE_GROUP: return launch_cheby_r(d, L, p.force_retry, a, st);
        case LE_GENERAL:
            return for_dim<1, MAX_D>(d, [&](auto K) {
                hipLaunchKernelGGL(cheby_kernel<decltype(K)::value>, dim3((unsigned)L.grid), dim3(L.block), L.lds, st, B, m_max,
                                   L.gs, A, b, mrows, r, xc, status);
            });
        default: return 2;
    }
}

// `ho`: where the launch leaves what the verifier takes (plan_bbox's hand-over mode says which of it), or nullptr
int launch_bbox(long long B, int m_max, int d, const double* A, const double* b, const int* mrows, double* lb,
                double* ub, int* status, hipStream_t st, const BoxHandover* ho) {
    const BoxPlan p = plan_bbox(B, m_max, d, lp_env());
    const BoxArgs a{B, m_max, A, b, mrows, lb, ub, status, ho ? *ho : BoxHandover{nullptr, nullptr, nullptr}};
    switch (p.first.engine) {
        case LE_LANE: return launch_bbox_lane(d, p.first, a, st);
        case LE_WIDE: return launch_bbox_lazy(d, p.first, a, st);
        case LE_SPLIT:
        case LE_GROUP: return launch_bbox_r(d, p.first, p.force_retry, a, st);
        default: return 2;
    }
}

// compact == nullptr: all pairs into the n x n matrix adj; else pairs [p_lo, p_hi) into compact[p - p_lo]
int launch_adjacent(int n, int m_max, int d, const double* A, const double* b, const int* mrows, double inflate,
                    double thresh, unsigned char* adj, long long p_lo, long long p_hi, unsigned char* compact,
                    hipStream_t st, int cross_n1, void* careful_scratch) {
    const PairPlan p = plan_pairs(n, m_max, d, p_lo, p_hi, compact != nullptr, cross_n1, lp_env());
    const PairArgs a{n, m_max, A, b, mrows, inflate, thresh, adj, p.p_lo, p.p_hi, compact, cross_n1, careful_scratch ? 1 : 0};
    int rc;
    switch (p.first.engine) {
        case LE_EMPTY: return 0;
        case LE_WIDE: rc = launch_adjacent_w(d, p.first, a, st); break;
        case LE_GROUP: rc = launch_adjacent_r(d, p.first, p.force_retry, a, st); break;
        default: return 2;
    }
    if (rc == 0 && careful_scratch)
        launch_careful_pairs(n, m_max, d, A, b, mrows, inflate, thresh, adj, p.p_lo, p.p_hi, compact, cross_n1, careful_scratch, st);
    return rc;
}

// the listed pairs list[K][2] into out[K]
int launch_pair_list(int n, int m_max, int d, const double* A, const double* b, const int* mrows, double inflate, double thresh,
                     long long K, const int* list, unsigned char* out, hipStream_t st, void* careful_scratch) {
    const PairPlan p = plan_pair_list(n, m_max, d, K, lp_env());
    const PairArgs a{n, m_max, A, b, mrows, inflate, thresh, nullptr, 0, K, out, 0, careful_scratch ? 1 : 0, list};
    int rc;
    switch (p.first.engine) {
        case LE_EMPTY: return 0;
        case LE_WIDE: rc = launch_adjacent_w_list(d, p.first, a, st); break;
        case LE_GROUP: rc = launch_adjacent_r_list(d, p.first, p.force_retry, a, st); break;
        default: return 2;
    }
    if (rc == 0 && careful_scratch)
        launch_careful_pairs(n, m_max, d, A, b, mrows, inflate, thresh, nullptr, 0, K, out, 0, careful_scratch, st, list);
    return rc;
}

}  // namespace plp
