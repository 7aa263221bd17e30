// plp_support.hip -- support_kernel<D, RV>: support functions of B polytopes in K directions each on the one-LP-per-lane
// engine, the rows of a polytope staged into LDS once for all its directions (plp_support.hpp: tiles, layout, statuses).
#include "plp_kernels.hpp"
#include "plp_support.hpp"

namespace plp {

constexpr int SUP_BLOCK = 64;   // one wavefront per workgroup

// np polytopes per workgroup (a power of two, <= support::np_cap(RV)), 64 / np lanes each.
// C: [K][D] (c_shared) or [B][K][D];  val / status [B][K], x [B][K][D] or nullptr.
template <int D, int RV>
__global__ __launch_bounds__(SUP_BLOCK) void support_kernel(const long long B, const int m_max, const double* __restrict__ Ag,
                                                            const double* __restrict__ bg, const int* __restrict__ mrows,
                                                            const int K, const double* __restrict__ Cg, const int c_shared,
                                                            const double* __restrict__ xcg, const int np,
                                                            double* __restrict__ val, double* __restrict__ xout,
                                                            int* __restrict__ status) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    double* sA = reinterpret_cast<double*>(smem_raw);   // [RV * D][np]
    double* sbeta = sA + (size_t)RV * D * np;           // [RV][np]
    const int lane = threadIdx.x;
    const long long tile = (long long)blockIdx.x * np;  // first polytope of this workgroup
    const int ntile = (B - tile) < np ? (int)(B - tile) : np;
    // ---- stage: slot (row i, polytope p) by lane, consecutive lanes on consecutive polytopes (LDS stores without a
    // bank conflict); rows i >= m[p] and polytopes past the batch as zero rows with beta = 0
    for (int s = lane; s < RV * np; s += SUP_BLOCK) {
        const int p = s % np, i = s / np;
        const bool pv = p < ntile;
        const long long P = tile + (pv ? p : 0);
        int m = mrows ? mrows[P] : m_max;
        m = m < 0 ? 0 : (m > m_max ? m_max : m);
        const bool live = pv & (i < m);
        double a[D], xc[D];
        const double* src = Ag + (P * m_max + (live ? i : 0)) * D;
#pragma unroll
        for (int k = 0; k < D; ++k) {
            a[k] = live ? src[k] : 0.0;
            xc[k] = live ? xcg[P * D + k] : 0.0;
        }
        const double bi = live ? bg[P * m_max + i] : 0.0;
        const double beta = live ? support::beta_of<D>(a, bi, xc) : 0.0;
#pragma unroll
        for (int k = 0; k < D; ++k) sA[(i * D + k) * np + p] = a[k];
        sbeta[i * np + p] = beta;
    }
    __syncthreads();
    // ---- one LP per lane: polytope p, direction j of round rd
    const int L = SUP_BLOCK / np;
    const int p = lane / L, jl = lane % L;
    const bool pv = p < ntile;
    const long long P = tile + (pv ? p : 0);
    int m = pv ? (mrows ? mrows[P] : m_max) : 0;
    m = m < 0 ? 0 : (m > m_max ? m_max : m);
    double xc[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int k = 0; k < D; ++k) xc[k] = pv ? xcg[P * D + k] : 0.0;
    const int rounds = (K + L - 1) / L;   // (the same for every lane)
    for (int rd = 0; rd < rounds; ++rd) {
        const int j = rd * L + jl;
        const bool go = pv & (j < K);
        const long long lp = P * K + (go ? j : 0);
        double c[4] = {0.0, 0.0, 0.0, 0.0};
        const double* csrc = Cg + (c_shared ? (long long)(go ? j : 0) : lp) * D;
#pragma unroll
        for (int k = 0; k < D; ++k) c[k] = go ? csrc[k] : 0.0;
        double v, x[4];
        int st;
        support::solve_one<D, RV>(sA + p, sbeta + p, np, m, c, xc, go, [](bool q) { return __any(q) != 0; }, v, x, st);
        if (go) {
            val[lp] = v;
            status[lp] = st;
            if (xout) {
#pragma unroll
                for (int k = 0; k < D; ++k) xout[lp * D + k] = x[k];
            }
        }
    }
}

template <int D>
static int launch_support_d(long long B, int m_max, const double* A, const double* b, const int* mrows, int K, const double* C,
                            int c_shared, const double* xc, double* val, double* x, int* status, hipStream_t st) {
    const int rv = support::row_slots(m_max);
    const int np = support::polytopes_per_group(K, rv);
    const long long blocks = (B + np - 1) / np;
    if (blocks > 2147483647ll) return 2;
#define PLP_SUP(RV)                                                                                                          \
    hipLaunchKernelGGL((support_kernel<D, RV>), dim3((unsigned)blocks), dim3(SUP_BLOCK), support::lds_bytes(D, RV, np), st, B, \
                       m_max, A, b, mrows, K, C, c_shared, xc, np, val, x, status)
    if (rv == 16) PLP_SUP(16);
    else if (rv == 32) PLP_SUP(32);
    else PLP_SUP(64);
#undef PLP_SUP
    return 0;
}

// val[B][K], x[B][K][d] (or nullptr), status[B][K] of plp_support_batch; 0 when launched, 2 for a size the kernel does not take
int launch_support(long long B, int m_max, int d, const double* A, const double* b, const int* mrows, int K, const double* C,
                   int c_shared, const double* xc, double* val, double* x, int* status, hipStream_t st) {
    if (B < 1 || K < 1 || B * (long long)K > 2147483647ll || support::row_slots(m_max) == 0) return 2;
    switch (d) {
        case 1: return launch_support_d<1>(B, m_max, A, b, mrows, K, C, c_shared, xc, val, x, status, st);
        case 2: return launch_support_d<2>(B, m_max, A, b, mrows, K, C, c_shared, xc, val, x, status, st);
        case 3: return launch_support_d<3>(B, m_max, A, b, mrows, K, C, c_shared, xc, val, x, status, st);
        case 4: return launch_support_d<4>(B, m_max, A, b, mrows, K, C, c_shared, xc, val, x, status, st);
        default: return 2;
    }
}

}  // namespace plp
