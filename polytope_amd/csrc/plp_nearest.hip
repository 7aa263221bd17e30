// plp_nearest.hip -- nearest_kernel<D, RV>: nearest points of B polytopes to K points each, one dual active-set walk per
// lane, the rows of a polytope staged into LDS once per (tile, K-chunk) at unit norm (plp_nearest.hpp: the walk, the end
// checks, the statuses; plp_support.hpp: the tiles and the LDS layout).
#include "plp_kernels.hpp"
#include "plp_nearest.hpp"

namespace plp {

constexpr int NEAR_BLOCK = 64;   // one wavefront per workgroup

// np polytopes per workgroup (a power of two, <= support::np_cap(RV)), 64 / np lanes each; blockIdx.y: the K-chunk, `rounds`
// rounds of 64 / np points per polytope.  X: [K][D] (x_shared) or [B][K][D];  dist / status [B][K]; xout / lam [B][K][D] and
// face [B][K] or nullptr.
template <int D, int RV>
__global__ __launch_bounds__(NEAR_BLOCK) void nearest_kernel(const long long B, const int m_max, const double* __restrict__ Ag,
                                                             const double* __restrict__ bg, const int* __restrict__ mrows,
                                                             const int K, const double* __restrict__ Xg, const int x_shared,
                                                             const int np, const int rounds, double* __restrict__ dist,
                                                             double* __restrict__ xout, unsigned long long* __restrict__ face,
                                                             double* __restrict__ lamout, int* __restrict__ status) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    double* sN = reinterpret_cast<double*>(smem_raw);   // [RV * D][np]
    double* sbeta = sN + (size_t)RV * D * np;           // [RV][np]
    double* snrm = sbeta + (size_t)RV * np;             // [RV][np]
    const int lane = threadIdx.x;
    const long long tile = (long long)blockIdx.x * np;  // first polytope of this workgroup
    const int ntile = (B - tile) < np ? (int)(B - tile) : np;
    // ---- stage: slot (row i, polytope p) by lane, consecutive lanes on consecutive polytopes; rows i >= m[p] and polytopes
    // past the batch as zero rows (nothing of them is read)
    for (int s = lane; s < RV * np; s += NEAR_BLOCK) {
        const int p = s % np, i = s / np;
        const bool pv = p < ntile;
        const long long P = tile + (pv ? p : 0);
        int m = mrows ? mrows[P] : m_max;
        m = m < 0 ? 0 : (m > m_max ? m_max : m);
        const bool live = pv & (i < m);
        double a[D], n[D], beta, nrm;
        const double* src = Ag + (P * m_max + (live ? i : 0)) * D;
#pragma unroll
        for (int k = 0; k < D; ++k) a[k] = live ? src[k] : 0.0;
        const double bi = live ? bg[P * m_max + i] : 0.0;
        nearest::stage_row<D>(a, bi, live, n, beta, nrm);
#pragma unroll
        for (int k = 0; k < D; ++k) sN[(i * D + k) * np + p] = n[k];
        sbeta[i * np + p] = beta;
        snrm[i * np + p] = nrm;
    }
    __syncthreads();
    // ---- one problem per lane: polytope p, point j of round rd of this chunk
    const int L = NEAR_BLOCK / np;
    const int p = lane / L, jl = lane % L;
    const bool pv = p < ntile;
    const long long P = tile + (pv ? p : 0);
    int m = pv ? (mrows ? mrows[P] : m_max) : 0;
    m = m < 0 ? 0 : (m > m_max ? m_max : m);
    const long long j0 = (long long)blockIdx.y * rounds * L;
    for (int rd = 0; rd < rounds; ++rd) {
        const long long j = j0 + (long long)rd * L + jl;
        if (!(pv & (j < K))) continue;
        const long long q = P * K + j;
        const double* psrc = Xg + (x_shared ? j : q) * D;
        double pt[D], x[D], lam[D], dd;
#pragma unroll
        for (int k = 0; k < D; ++k) pt[k] = psrc[k];
        uint64_t fc;
        int st;
        nearest::solve_one<D, RV>(sN + p, sbeta + p, snrm + p, np, m, pt, dd, x, fc, lam, st);
        dist[q] = dd;
        status[q] = st;
        if (face) face[q] = fc;
        if (xout) {
#pragma unroll
            for (int k = 0; k < D; ++k) xout[q * D + k] = x[k];
        }
        if (lamout) {
#pragma unroll
            for (int k = 0; k < D; ++k) lamout[q * D + k] = lam[k];
        }
    }
}

template <int D>
static int launch_nearest_d(long long B, int m_max, const double* A, const double* b, const int* mrows, int K, const double* X,
                            int x_shared, double* dist, double* x, unsigned long long* face, double* lam, int* status,
                            hipStream_t st) {
    const int rv = nearest::row_slots(m_max);
    const int np = nearest::polytopes_per_group(K, rv);
    const int L = NEAR_BLOCK / np;
    const int rounds = nearest::chunk_rounds(K, L);
    const long long blocks = (B + np - 1) / np;
    const long long chunks = ((long long)K + (long long)rounds * L - 1) / ((long long)rounds * L);
    if (blocks > 2147483647ll || chunks > 65535) return 2;
#define PLP_NEAR(RV)                                                                                                       \
    hipLaunchKernelGGL((nearest_kernel<D, RV>), dim3((unsigned)blocks, (unsigned)chunks), dim3(NEAR_BLOCK),               \
                       nearest::lds_bytes(D, RV, np), st, B, m_max, A, b, mrows, K, X, x_shared, np, rounds, dist, x, face, \
                       lam, status)
    if (rv == 16) PLP_NEAR(16);
    else if (rv == 32) PLP_NEAR(32);
    else PLP_NEAR(64);
#undef PLP_NEAR
    return 0;
}

// dist[B][K], x[B][K][d], face[B][K], lam[B][K][d] (each or nullptr), status[B][K] of plp_nearest_batch; 0 when launched, 2 for
// a size the kernel does not take
int launch_nearest(long long B, int m_max, int d, const double* A, const double* b, const int* mrows, int K, const double* X,
                   int x_shared, double* dist, double* x, unsigned long long* face, double* lam, int* status, hipStream_t st) {
    if (B < 1 || K < 1 || B * (long long)K > 2147483647ll || nearest::row_slots(m_max) == 0) return 2;
    switch (d) {
        case 1: return launch_nearest_d<1>(B, m_max, A, b, mrows, K, X, x_shared, dist, x, face, lam, status, st);
        case 2: return launch_nearest_d<2>(B, m_max, A, b, mrows, K, X, x_shared, dist, x, face, lam, status, st);
        case 3: return launch_nearest_d<3>(B, m_max, A, b, mrows, K, X, x_shared, dist, x, face, lam, status, st);
        case 4: return launch_nearest_d<4>(B, m_max, A, b, mrows, K, X, x_shared, dist, x, face, lam, status, st);
        default: return 2;
    }
}

}  // namespace plp
