// plp_nearest.hip -- nearest_kernel<D, RV>: nearest points of B polytopes to K points each, one dual active-set walk per
// lane, the rows of a polytope staged into LDS once per (tile, K-chunk) at unit norm (plp_nearest.hpp: the walk, the end
// checks, the statuses; plp_row_tile.hpp: the tiles, the LDS layout, the frame of the kernel).
#include "plp_kernels.hpp"
#include "plp_nearest.hpp"

namespace plp {

// np polytopes per workgroup; blockIdx.y: the K-chunk, `rounds` rounds of 64 / np points per polytope (plp_row_tile.hpp).
// X: [K][D] (x_shared) or [B][K][D];  dist / status [B][K]; xout / lam [B][K][D] and face [B][K] or nullptr.
template <int D, int RV>
__global__ __launch_bounds__(rowtile::BLOCK) void nearest_kernel(const long long B, const int m_max, const double* __restrict__ Ag,
                                                                 const double* __restrict__ bg, const int* __restrict__ mrows,
                                                                 const int K, const double* __restrict__ Xg, const int x_shared,
                                                                 const int np, const int rounds, double* __restrict__ dist,
                                                                 double* __restrict__ xout, unsigned long long* __restrict__ face,
                                                                 double* __restrict__ lamout, int* __restrict__ status) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    double* sN = reinterpret_cast<double*>(smem_raw);   // n_i, then the planes of beta_i and |a_i| (zero rows beyond m)
    const rowtile::Lane ln = rowtile::stage<D, RV, 2>(
        sN, B, m_max, Ag, bg, mrows, np,
        [](const double(&a)[D], const double bi, const bool live, const long long, double(&n)[D], double(&s)[2]) {
            nearest::stage_row<D>(a, bi, live, n, s[0], s[1]);
        });
    const double *sbeta = rowtile::plane<D, RV>(sN, np, 0), *snrm = rowtile::plane<D, RV>(sN, np, 1);
    // ---- one problem per lane
    rowtile::for_rounds(ln, K, rounds, [&](const bool go, const long long j, const long long q) {
        if (!go) return;
        const double* psrc = Xg + (x_shared ? j : q) * D;
        double pt[D], x[D], lam[D], dd;
#pragma unroll
        for (int k = 0; k < D; ++k) pt[k] = psrc[k];
        uint64_t fc;
        int st;
        nearest::solve_one<D, RV>(sN + ln.p, sbeta + ln.p, snrm + ln.p, np, ln.m, pt, dd, x, fc, lam, st);
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
    });
}

// dist[B][K], x[B][K][d], face[B][K], lam[B][K][d] (each or nullptr), status[B][K] of plp_nearest_batch; 0 when launched, 2 for
// a size the kernel does not take
int launch_nearest(long long B, int m_max, int d, const double* A, const double* b, const int* mrows, int K, const double* X,
                   int x_shared, double* dist, double* x, unsigned long long* face, double* lam, int* status, hipStream_t st) {
    const int rv = rowtile::row_slots(m_max);
    if (B < 1 || K < 1 || B * (long long)K > 2147483647ll || rv == 0) return 2;
    const rowtile::Grid g = rowtile::grid(B, K, rv, nearest::K_ROUNDS);
    if (!g.fits()) return 2;
    return rowtile::dispatch(d, rv, [&](auto dim, auto rows) {
        constexpr int D = decltype(dim)::value, RV = decltype(rows)::value;
        hipLaunchKernelGGL((nearest_kernel<D, RV>), dim3((unsigned)g.blocks, (unsigned)g.chunks), dim3(rowtile::BLOCK),
                           rowtile::lds_bytes(D, RV, g.np, 2), st, B, m_max, A, b, mrows, K, X, x_shared, g.np, g.rounds, dist, x,
                           face, lam, status);
    });
}

}  // namespace plp
