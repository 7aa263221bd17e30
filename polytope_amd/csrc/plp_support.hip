// plp_support.hip -- support_kernel<D, RV>: support functions of B polytopes in K directions each on the one-LP-per-lane
// engine, the rows of a polytope staged into LDS once for all its directions (plp_row_tile.hpp: tiles, layout, the frame of
// the kernel; plp_support.hpp: the LP, the end checks, the statuses).
#include "plp_kernels.hpp"
#include "plp_support.hpp"

namespace plp {

// np polytopes per workgroup, `rounds` rounds of 64 / np directions per polytope (plp_row_tile.hpp; the launcher asks for one
// K-chunk of all rounds: gridDim.y == 1).  C: [K][D] (c_shared) or [B][K][D];  val / status [B][K], x [B][K][D] or nullptr.
template <int D, int RV>
__global__ __launch_bounds__(rowtile::BLOCK) void support_kernel(const long long B, const int m_max, const double* __restrict__ Ag,
                                                                 const double* __restrict__ bg, const int* __restrict__ mrows,
                                                                 const int K, const double* __restrict__ Cg, const int c_shared,
                                                                 const double* __restrict__ xcg, const int np, const int rounds,
                                                                 double* __restrict__ val, double* __restrict__ xout,
                                                                 int* __restrict__ status) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    double* sA = reinterpret_cast<double*>(smem_raw);   // a_i, then the plane of beta_i (zero rows with beta = 0 beyond m)
    const rowtile::Lane ln = rowtile::stage<D, RV, 1>(
        sA, B, m_max, Ag, bg, mrows, np,
        [&](const double(&a)[D], const double bi, const bool live, const long long P, double(&n)[D], double(&s)[1]) {
            double xc[D];
#pragma unroll
            for (int k = 0; k < D; ++k) {
                n[k] = a[k];
                xc[k] = live ? xcg[P * D + k] : 0.0;
            }
            s[0] = live ? support::beta_of<D>(a, bi, xc) : 0.0;
        });
    const double* sbeta = rowtile::plane<D, RV>(sA, np, 0);
    double xc[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int k = 0; k < D; ++k) xc[k] = ln.pv ? xcg[ln.P * D + k] : 0.0;
    // ---- one LP per lane; a lane without one still takes part in the wavefront's votes
    rowtile::for_rounds(ln, K, rounds, [&](const bool go, const long long j, const long long lp) {
        double c[4] = {0.0, 0.0, 0.0, 0.0};
        const double* csrc = Cg + (c_shared ? j : lp) * D;
#pragma unroll
        for (int k = 0; k < D; ++k) c[k] = go ? csrc[k] : 0.0;
        double v, x[4];
        int st;
        support::solve_one<D, RV>(sA + ln.p, sbeta + ln.p, np, ln.m, c, xc, go, [](bool q) { return __any(q) != 0; }, v, x, st);
        if (go) {
            val[lp] = v;
            status[lp] = st;
            if (xout) {
#pragma unroll
                for (int k = 0; k < D; ++k) xout[lp * D + k] = x[k];
            }
        }
    });
}

// val[B][K], x[B][K][d] (or nullptr), status[B][K] of plp_support_batch; 0 when launched, 2 for a size the kernel does not take
int launch_support(long long B, int m_max, int d, const double* A, const double* b, const int* mrows, int K, const double* C,
                   int c_shared, const double* xc, double* val, double* x, int* status, hipStream_t st) {
    const int rv = rowtile::row_slots(m_max);
    if (B < 1 || K < 1 || B * (long long)K > 2147483647ll || rv == 0) return 2;
    const rowtile::Grid g = rowtile::grid(B, K, rv, 0);   // (one K-chunk: DESIGN.md 7)
    if (!g.fits()) return 2;
    return rowtile::dispatch(d, rv, [&](auto dim, auto rows) {
        constexpr int D = decltype(dim)::value, RV = decltype(rows)::value;
        hipLaunchKernelGGL((support_kernel<D, RV>), dim3((unsigned)g.blocks, (unsigned)g.chunks), dim3(rowtile::BLOCK),
                           rowtile::lds_bytes(D, RV, g.np, 1), st, B, m_max, A, b, mrows, K, C, c_shared, xc, g.np, g.rounds, val, x,
                           status);
    });
}

}  // namespace plp
