// plp_projhull.hip -- projhull_kernel<D, K>: the iterative-hull projection of B polytopes onto K of their coordinates in one
// launch, one polytope per wavefront (plp_projhull.hpp: the contract, the caps, the rule).  The rows are read from global
// memory once and stay in LDS as (a_i, b_i - a_i.xc); the points, the facets, the confirmed facets and the rule's state live
// in LDS too.  Lane 0 runs projhull::step(); what it asks for, the whole wavefront answers: an LP on the
// one-LP-per-wavefront engine (wide::solve_dense_point, plp_wide.hpp), or the enumeration of the facets of the points held,
// 64 candidates at a time on the skeleton of hull_enum_kernel (wenum::wave_greedy_round, plp_enum.hpp).
#include "plp_kernels.hpp"
#include "plp_projhull.hpp"
#include "plp_wide.hpp"

namespace plp {

namespace {

// The wave twin of projhull::enumerate(): the same candidates in the same order, the same list.
template <int K>
__device__ __forceinline__ void enumerate_wave(projhull::State<K>& S, const int lane) {
    const int n = S.nv, f_max = S.f_max;
    const double* sq = S.q;
    const int* sidx = S.sidx;
    double* Ap = S.fnu;
    double* bp = S.foff;
    uint64_t* op = S.fon;
    const int T = wenum::candidates<K>(n);
    int cnt = 0;
    bool over = false, flat = false;
    for (int base = 0; base < T && !over; base += wenum::BLOCK) {
        const int rank = base + lane;
        double nu[K], off = 0.0;
        int idx[K];
        uint64_t w = 0;
#pragma unroll
        for (int k = 0; k < K; ++k) {
            nu[k] = 0.0;
            idx[k] = 0;
        }
        int kind = hullenum::CAND_NONE;
        if (rank < T) {
            wenum::unrank<K>(n, rank, idx);
            kind = hullenum::candidate<K>(sq, sidx, n, idx, nu, off, w);
        }
        const unsigned long long flatm = __ballot(kind == hullenum::CAND_FLAT);
        const int first_flat = flatm ? __ffsll((long long)flatm) - 1 : wenum::BLOCK;
        over = wenum::wave_greedy_round(
            lane, kind == hullenum::CAND_FACET && lane < first_flat, cnt, f_max,
            [&](const int q) {
                double a[K];
#pragma unroll
                for (int k = 0; k < K; ++k) a[k] = Ap[q * K + k];
                return hullenum::same<K>(nu, off, a, bp[q]);
            },
            [&](const int src) {
                double a[K];
#pragma unroll
                for (int k = 0; k < K; ++k) a[k] = __shfl(nu[k], src);
                return hullenum::same<K>(nu, off, a, __shfl(off, src));
            },
            [&](const int q) {
#pragma unroll
                for (int k = 0; k < K; ++k) Ap[q * K + k] = nu[k];
                bp[q] = off;
                op[q] = w;
            });
        if (flatm && !over) {   // (uniform)
            flat = true;
            break;
        }
    }
    if (lane == 0) {
        S.count = flat ? 0 : cnt;
        S.en_flat = flat ? 1 : 0;
        S.en_over = over ? 1 : 0;
    }
}

}  // namespace

// Workgroup (= wavefront) w, w + grid, ... takes polytope w.  d <= D: the columns d .. D - 1 are zero columns with zero
// cost, which never price in.
//   stage : lane i < m[p] reads row i and puts (a_i, beta_i = b_i - a_i.xc) into LDS / a register; only rows below m[p] are
//           read.  A live row with beta_i <= 0 or an entry that is not finite: PH_NOCENTRE, nothing is run
//   loop  : lane 0 steps the rule; the wavefront answers (see above)
//   write : the rows in the caller's coordinates, V, the tails (NaN), and by lane 0 count, nv, vmask, nlp, status
template <int D, int K>
__global__ __launch_bounds__(64) void projhull_kernel(const long long B, const int m_max, const int d, const double* __restrict__ Ag,
                                                      const double* __restrict__ bg, const int* __restrict__ mrows, const int k0,
                                                      const int k1, const int k2, const double* __restrict__ xcg, const int f_max,
                                                      const int max_lps, double* __restrict__ Ao, double* __restrict__ bo,
                                                      unsigned long long* __restrict__ on, int* __restrict__ count,
                                                      double* __restrict__ Vo, int* __restrict__ nvo, double* Xo,
                                                      unsigned long long* __restrict__ vmask, int* __restrict__ nlp,
                                                      int* __restrict__ status) {
    __shared__ __attribute__((aligned(16))) double sA[64 * D];
    __shared__ double sxc[D];
    __shared__ wide::WideShared<D> sh;
    __shared__ projhull::State<K> S;
    const int lane = threadIdx.x;
    const int keep[3] = {k0, k1, k2};
    for (long long p = blockIdx.x; p < B; p += gridDim.x) {
        __syncthreads();   // (the last polytope's reads of the blocks are done)
        int m = mrows ? mrows[p] : m_max;
        m = m < 0 ? 0 : (m > m_max ? m_max : m);
        const bool has = lane < m;
        // ---- stage
        double dotc = 0.0;
        bool finite = true;
#pragma unroll
        for (int k = 0; k < D; ++k) {
            const bool in = k < d;
            const double v = (has & in) ? Ag[(p * m_max + lane) * d + k] : 0.0;
            const double x = in ? xcg[p * d + k] : 0.0;
            sA[lane * D + k] = v;
            if (lane == 0) sxc[k] = x;
            dotc = k == 0 ? v * x : fma(v, x, dotc);
            finite = finite & isfinite(v);
        }
        const double bi = has ? bg[p * m_max + lane] : 0.0;
        const double beta = has ? bi - dotc : 0.0;
        const bool bad = has & !(finite & (beta > 0.0) & isfinite(beta));
        const bool nocentre = (__ballot(bad) != 0ull) | (m < 1);
        const double babs = wenum::wave_max(has ? fabs(beta) : 0.0);
        double* Xp = Xo ? Xo + p * projhull::MAX_POINTS * d : nullptr;
        if (lane == 0) {
            projhull::begin(S, d, keep, f_max, max_lps, babs);
            if (nocentre) projhull::done(S, projhull::PH_NOCENTRE);
        }
        __syncthreads();
        // ---- the rule
        while (!nocentre) {
            if (lane == 0) projhull::step(S, Xp);
            __syncthreads();
            const int req = S.req;
            if (req == projhull::REQ_DONE) break;
            if (req == projhull::REQ_LP) {
                // min (-dir) . y over the staged rows: lane j holds the cost of column j
                double cj = 0.0;
#pragma unroll
                for (int t = 0; t < K; ++t) cj = (lane == keep[t]) ? -S.dir[t] : cj;
                double y[D], negz = 0.0;
                const int st = wide::solve_dense_point<D>(lane, m, sA, cj, beta, has, negz, sh, y);
                double r = 0.0;
#pragma unroll
                for (int k = 0; k < D; ++k) r = r + sA[lane * D + k] * y[k];
                const double v = has ? r - beta : -__builtin_inf();
                const bool isnan_any = __ballot(v != v) != 0ull;
                const double viol = isnan_any ? __builtin_nan("") : wenum::wave_max(v);
                if (lane == 0) {
                    S.lp_status = st;
                    S.lp_viol = viol;
#pragma unroll
                    for (int k = 0; k < D; ++k)
                        if (k < d) S.lp_x[k] = y[k] + sxc[k];
                }
            } else {
                enumerate_wave<K>(S, lane);
            }
            __syncthreads();
        }
        // ---- write
        projhull::finish_rows<K>(S, f_max, Ao + p * f_max * K, bo + p * f_max, (uint64_t*)(on + p * f_max), lane, 64);
        projhull::finish_points<K>(S, Vo + p * projhull::MAX_POINTS * K, Xp, lane, 64);
        const unsigned long long vm = __ballot(projhull::vertex_bit<K>(S, lane));
        if (lane == 0) {
            count[p] = projhull::out_count(S);
            nvo[p] = S.nv;
            vmask[p] = vm;
            nlp[p] = S.nlp;
            status[p] = S.status;
        }
    }
}

// 0 when launched, 2 for a size the kernel does not take.  keep: k HOST integers, 0-based and increasing, below d.
int launch_projhull(long long B, int m_max, int d, int k, const double* A, const double* b, const int* mrows, const int* keep,
                    const double* xc, int f_max, int max_lps, double* Ao, double* bo, unsigned long long* on, int* count, double* V,
                    int* nv, double* X, unsigned long long* vmask, int* nlp, int* status, hipStream_t st) {
    if (B < 1 || B > 2147483647ll || m_max < 0 || m_max > projhull::MAX_ROWS) return 2;
    if (k < 1 || k > projhull::MAX_K || d < k || d > projhull::MAX_D || f_max < 1 || f_max > projhull::F_CAP) return 2;
    int kk[3] = {-1, -1, -1};
    for (int t = 0; t < k; ++t) {
        if (keep[t] < 0 || keep[t] >= d || (t && keep[t] <= keep[t - 1])) return 2;
        kk[t] = keep[t];
    }
    const long long cap = 1ll << 16;
    const unsigned grid = (unsigned)(B < cap ? B : cap);
#define PLP_PH(DD, KK)                                                                                                      \
    hipLaunchKernelGGL((projhull_kernel<DD, KK>), dim3(grid), dim3(64), 0, st, B, m_max, d, A, b, mrows, kk[0], kk[1], kk[2], xc, \
                       f_max, max_lps, Ao, bo, on, count, V, nv, X, vmask, nlp, status)
#define PLP_PH_D(DD)                             \
    do {                                         \
        if (k == 1) PLP_PH(DD, 1);               \
        else if (k == 2) PLP_PH(DD, 2);          \
        else PLP_PH(DD, 3);                      \
    } while (0)
    // d is padded up to the next instance
    if (d <= 4) PLP_PH_D(4);
    else if (d <= 8) PLP_PH_D(8);
    else if (d <= 12) PLP_PH_D(12);
    else PLP_PH_D(16);
#undef PLP_PH_D
#undef PLP_PH
    return 0;
}

}  // namespace plp
