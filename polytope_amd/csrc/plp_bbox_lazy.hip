// plp_bbox_lazy.hip -- fused bounding boxes, one polytope of up to 64 rows per wavefront (polytope/polytope.py:1314-1411):
// the Chebyshev LP on the one-LP-per-wavefront engine (plp_wide.hpp), then the 2d LPs min / max x_k from its centre
//   WDENSE (d = 5..13): on the same dense engine (wide::solve_dense: wave-uniform pivots, Bland's rule inside),
//   otherwise (d = 14..16): WITHOUT a stored dictionary (plp_lazy.hpp).
// d = 9..16 always come here, d = 5..8 by the rule of plan_bbox (plp_lp_plan.hpp: the lane-group kernel bbox_r_kernel holds
// one or two polytopes of more than 32 rows per wavefront and pays select chains for the pivot column).  Same contract as bbox_r_kernel
// (plp_cheby_r_impl.hpp, d <= 8): status 0 = lb / ub hold the box (+-inf where an LP is unbounded, :1376 / :1398),
// status 1 = not handled here (empty / flat / unbounded-ball polytopes, LPs that ask for Bland's rule or run past the
// step limit): the caller solves the generic LPs for those.
#include "plp_lp_launch.hpp"
#include "plp_lazy.hpp"
#include "plp_reduce_rules.hpp"
#include "plp_wide.hpp"

namespace plp {

template <int D, bool WDENSE>
__global__ __launch_bounds__(64, 3) void bbox_lazy_kernel(long long B, int m_max, const double* __restrict__ A,
                                                          const double* __restrict__ b, const int* __restrict__ mrows,
                                                          double* __restrict__ lb, double* __restrict__ ub,
                                                          int* __restrict__ status, signed char* __restrict__ basis8,
                                                          double* __restrict__ centre) {
    constexpr int NC = D + 1;
    __shared__ __attribute__((aligned(16))) double sA[64 * D];
    __shared__ wide::WideShared<NC> sh;
    const int lane = threadIdx.x;
    const long long p = blockIdx.x;
    if (p >= B) return;
    const int m = mrows ? mrows[p] : m_max;
    const bool has = lane < m;
    // ---- F1 (plp_wide.hpp); my row also goes to LDS for the box LPs
    const double bi = has ? b[p * m_max + lane] : 0.0;
    typename wide::RowVec<NC>::type Tv;
    double T16;
    wide::ChebyRow c;
    wide::cheby_setup<D>(Tv, T16, c, lane, has, [&](int k) { return A[(p * m_max + lane) * D + k]; }, [&]() { return bi; }, sh);
#pragma unroll
    for (int k = 0; k < D; ++k) sA[lane * D + k] = ROW_GET(k);
    __syncthreads();
    const int st = wide::cheby_run<D>(Tv, T16, c, lane, m, sh, m > 64);
    double x[NC];
    wide::cheby_point<D>(c, x);
    const bool ok = (st == ST_OPT) & (x[D] >= rule::BBOX_MIN_R);
    bool handed = !ok;
    // ---- my slack at the centre (bbox_r_kernel: s by an fma chain, beta = max(b - s, 0))
    double s = 0.0;
#pragma unroll
    for (int k = 0; k < D; ++k) s = fma(has ? sA[lane * D + k] : 0.0, ok ? x[k] : 0.0, s);
    const double be0 = (ok & has) ? fmax(bi - s, 0.0) : 0.0;
    using rule::qnan;
    for (int it = 0; it < 2 * D; ++it) {  // lower_0, upper_0, lower_1, upper_1, ...
        const int kx = it >> 1;
        const bool up = it & 1;
        double xck = 0.0;
#pragma unroll
        for (int k = 0; k < D; ++k) xck = (k == kx) ? x[k] : xck;
        double val = qnan;
        if (__builtin_amdgcn_readfirstlane((int)ok)) {
            double negz = 0.0;
            int s2;
            signed char* bo = basis8 ? basis8 + ((size_t)p * 2 * D + it) * D : nullptr;  // the LP's final basis, for the verifier
            if constexpr (WDENSE)
                s2 = wide::solve_dense<D>(lane, m, sA, (lane == kx) ? (up ? -1.0 : 1.0) : 0.0, be0, has, negz,
                                          *reinterpret_cast<wide::WideShared<D>*>(&sh), bo);
            else
                s2 = lazy::solve<D>(lane, m, sA, (lane == kx) ? (up ? -1.0 : 1.0) : 0.0, be0, has, negz, bo);
            bool bad;
            val = rule::box_value(s2, up, rule::box_optimum(up, xck, negz), bad);
            handed = handed | bad;
        }
        if (lane == 0) (up ? ub : lb)[p * D + kx] = ok ? val : qnan;
    }
    if (lane == 0) status[p] = handed ? 1 : 0;
    if (centre && lane == 0) {
#pragma unroll
        for (int k = 0; k < D; ++k) centre[(size_t)p * D + k] = ok ? x[k] : qnan;
    }
}

// ---- small batches: NW wavefronts per polytope (the pattern of reduce_wsplit_kernel, plp_reduce_r_impl.hpp).  One workgroup
// per polytope: wavefront 0 runs F1 and leaves the centre in LDS, then wavefront w solves every NW-th of the 2d box LPs on the
// rows they share -- each LP exactly as in bbox_lazy_kernel (same engine, same set-up): lb / ub / status bit for bit.
template <int D, int NW, bool WDENSE>
__global__ __launch_bounds__(64 * NW) void bbox_wsplit_kernel(long long B, int m_max, const double* __restrict__ A,
                                                              const double* __restrict__ b, const int* __restrict__ mrows,
                                                              double* __restrict__ lb, double* __restrict__ ub,
                                                              int* __restrict__ status, signed char* __restrict__ basis8,
                                                              double* __restrict__ centre) {
    constexpr int NC = D + 1;
    __shared__ __attribute__((aligned(16))) double sA[64 * D];
    __shared__ wide::WideShared<NC> shw[NW];
    __shared__ double sx[NC + 1];
    __shared__ unsigned sflag[2];   // [0]: F1 gave a usable ball, [1]: some LP was handed back
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const long long p = blockIdx.x;
    if (p >= B) return;
    const int m = mrows ? mrows[p] : m_max;
    const bool has = lane < m;
    double bi = 0.0;
    if (w == 0) {
        // ---- F1 (plp_wide.hpp); my row also goes to LDS for the box LPs
        wide::WideShared<NC>& sh = shw[0];
        bi = has ? b[p * m_max + lane] : 0.0;
        typename wide::RowVec<NC>::type Tv;
        double T16;
        wide::ChebyRow c;
        wide::cheby_setup<D>(Tv, T16, c, lane, has, [&](int k) { return A[(p * m_max + lane) * D + k]; }, [&]() { return bi; }, sh);
#pragma unroll
        for (int k = 0; k < D; ++k) sA[lane * D + k] = ROW_GET(k);
        wide::wave_sync();
        const int st = wide::cheby_run<D>(Tv, T16, c, lane, m, sh, m > 64);
        double xf[NC];
        wide::cheby_point<D>(c, xf);
        const double xr = xf[D];
        if (lane == 0) {
#pragma unroll
            for (int j = 0; j < NC; ++j) sx[j] = xf[j];
        }
        if (lane == 0) {
            sflag[0] = ((st == ST_OPT) & (xr >= rule::BBOX_MIN_R)) ? 1u : 0u;
            sflag[1] = 0u;
        }
    }
    __syncthreads();
    if (w != 0) bi = has ? b[p * m_max + lane] : 0.0;
    const bool ok = sflag[0] != 0u;
    double x[D];
#pragma unroll
    for (int k = 0; k < D; ++k) x[k] = sx[k];
    // ---- my slack at the centre (bbox_r_kernel: s by an fma chain, beta = max(b - s, 0))
    double s = 0.0;
#pragma unroll
    for (int k = 0; k < D; ++k) s = fma(has ? sA[lane * D + k] : 0.0, ok ? x[k] : 0.0, s);
    const double be0 = (ok & has) ? fmax(bi - s, 0.0) : 0.0;
    using rule::qnan;
    bool handed = false;
    for (int it = w; it < 2 * D; it += NW) {  // lower_0, upper_0, lower_1, upper_1, ...: wavefront w every NW-th
        const int kx = it >> 1;
        const bool up = it & 1;
        double xck = 0.0;
#pragma unroll
        for (int k = 0; k < D; ++k) xck = (k == kx) ? x[k] : xck;
        double val = qnan;
        if (__builtin_amdgcn_readfirstlane((int)ok)) {   // (the same in every lane, and said so: the LP runs on full wavefronts)
            double negz = 0.0;
            int s2;
            signed char* bo = basis8 ? basis8 + ((size_t)p * 2 * D + it) * D : nullptr;  // the LP's final basis, for the verifier
            if constexpr (WDENSE)
                s2 = wide::solve_dense<D>(lane, m, sA, (lane == kx) ? (up ? -1.0 : 1.0) : 0.0, be0, has, negz,
                                          *reinterpret_cast<wide::WideShared<D>*>(&shw[w]), bo);
            else
                s2 = lazy::solve<D>(lane, m, sA, (lane == kx) ? (up ? -1.0 : 1.0) : 0.0, be0, has, negz, bo);
            bool bad;
            val = rule::box_value(s2, up, rule::box_optimum(up, xck, negz), bad);
            handed = handed | bad;
        }
        if (lane == 0) (up ? ub : lb)[p * D + kx] = ok ? val : qnan;
    }
    if (handed & (lane == 0)) atomicOr(&sflag[1], 1u);
    __syncthreads();
    if ((w == 0) & (lane == 0)) status[p] = (!ok | (sflag[1] != 0u)) ? 1 : 0;
    if (centre && (w == 0) && lane < D) centre[(size_t)p * D + lane] = ok ? sx[lane] : qnan;
}

// L.nw = 4: bbox_wsplit_kernel, a workgroup of four wavefronts per polytope; else bbox_lazy_kernel, one wavefront;
// L.dense: the 2d LPs with a stored dictionary.  Both leave the bases and the centres for the verifier.
int launch_bbox_lazy(int d, const LpLaunch& L, const BoxArgs& a, hipStream_t st) {
    return for_dim<5, MAX_D>(d, [&](auto K) {
        constexpr int D = decltype(K)::value;
#define PLP_BBW(KERNEL)                                                                                                       \
    hipLaunchKernelGGL(KERNEL, dim3((unsigned)L.grid), dim3(L.block), L.lds, st, a.B, a.m_max, a.A, a.b, a.mrows, a.lb, a.ub, \
                       a.status, a.ho.basis8, a.ho.centre)
        if (L.nw == 4) { if (L.dense) PLP_BBW((bbox_wsplit_kernel<D, 4, true>)); else PLP_BBW((bbox_wsplit_kernel<D, 4, false>)); }
        else if (L.dense) PLP_BBW((bbox_lazy_kernel<D, true>));
        else PLP_BBW((bbox_lazy_kernel<D, false>));
#undef PLP_BBW
    });
}

}  // namespace plp
