// plp_pair_dist.hip -- pair_dist_kernel<D, RV>: closest points and distances of listed cell pairs of a packed table, a GJK
// iteration per pair on top of the support LP of the lane engine (plp_pair_dist.hpp: the iteration, the end checks, the
// statuses; plp_support.hpp: the LP; plp_row_tile.hpp: the tile rules and the LDS layout).
//
// Tile: TWO LANES PER PAIR.  A workgroup (one wavefront) has np = polytopes_per_group(1, RV) = 64 / 32 / 16 row-tile slots at
// RV = 16 / 32 / 64 -- rowtile's K = 1 layout, one lane per slot -- and slot 2 s holds cell i, slot 2 s + 1 cell j of the
// tile's pair s, read through the pair list: a slot -> cell indirection, done here (rowtile::stage is left as it is).  A cell
// listed in several pairs of a tile is staged once per listing.  Lane 2 s walks cell i, lane 2 s + 1 cell j; each keeps its
// own side's support points and both keep the differences w_k, exchange their new support point, its value and the LP's
// status by a cross-lane move (lane ^ 1) and run the simplex step redundantly on the same numbers, so their control flow
// is the same and the answers are those of the host build, which works both cells in one call, bit for bit.
#include "plp_kernels.hpp"
#include "plp_pair_dist.hpp"

namespace plp {

// pairs int32[K][2]; dist / lb / status [K], x / y [K][D] (lb, x, y each or nullptr); np slots = np / 2 pairs per workgroup
template <int D, int RV>
__global__ __launch_bounds__(rowtile::BLOCK) void pair_dist_kernel(const int n, const int m_max, const double* __restrict__ Ag,
                                                                   const double* __restrict__ bg, const int* __restrict__ mrows,
                                                                   const double* __restrict__ xcg, const long long K,
                                                                   const int* __restrict__ pairs, const int np,
                                                                   double* __restrict__ dist, double* __restrict__ lbout,
                                                                   double* __restrict__ xout, double* __restrict__ yout,
                                                                   int* __restrict__ status) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    double* sA = reinterpret_cast<double*>(smem_raw);   // a_i, then the plane of beta_i (zero rows with beta = 0 beyond m)
    double* sbeta = rowtile::plane<D, RV>(sA, np, 0);
    const int lane = threadIdx.x;
    const long long t0 = (long long)blockIdx.x * (np / 2);   // first pair of this workgroup
    // the cell of slot p, or -1: a slot past the list, a pair that is not two different cells of [0, n)
    auto cell_of = [&](const int p, int& other) {
        const long long t = t0 + p / 2;
        other = -1;
        if (t >= K) return -1;
        const int i = pairs[2 * t], j = pairs[2 * t + 1];
        if (i < 0 || i >= n || j < 0 || j >= n || i == j) return -1;
        other = (p & 1) ? i : j;
        return (p & 1) ? j : i;
    };
    // ---- the rows of the tile's cells: slot (row i, slot p) by lane, consecutive lanes on consecutive slots
    for (int s = lane; s < RV * np; s += rowtile::BLOCK) {
        const int p = s % np, i = s / np;
        int other;
        const int cell = cell_of(p, other);
        const long long P = cell < 0 ? 0 : cell;
        const bool live = (cell >= 0) && (i < rowtile::clamp_rows(mrows ? mrows[P] : m_max, m_max));
        double a[D], xc[D];
        const double* src = Ag + (P * m_max + (live ? i : 0)) * D;
#pragma unroll
        for (int k = 0; k < D; ++k) {
            a[k] = live ? src[k] : 0.0;
            xc[k] = live ? xcg[P * D + k] : 0.0;
        }
        const double bi = live ? bg[P * m_max + i] : 0.0;
#pragma unroll
        for (int k = 0; k < D; ++k) sA[(i * D + k) * np + p] = a[k];
        sbeta[i * np + p] = live ? support::beta_of<D>(a, bi, xc) : 0.0;
    }
    __syncthreads();
    // ---- one cell of one pair per lane; a lane without one still takes part in the wavefront's votes
    const bool slot = lane < np;
    const int p = slot ? lane : 0, side = lane & 1;
    const long long t = t0 + p / 2;
    const bool listed = slot & (t < K);
    int other = -1;
    const int cell = slot ? cell_of(p, other) : -1;
    const bool go = cell >= 0;
    const int m = go ? rowtile::clamp_rows(mrows ? mrows[cell] : m_max, m_max) : 0;
    double xc[4] = {0.0, 0.0, 0.0, 0.0}, v0[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int k = 0; k < D; ++k) {
        xc[k] = go ? xcg[(long long)cell * D + k] : 0.0;
        const double xo = go ? xcg[(long long)other * D + k] : 0.0;
        v0[k] = side ? xo - xc[k] : xc[k] - xo;   // xc_i - xc_j on both lanes
    }
    const double *pA = sA + p, *pbeta = sbeta + p;
    auto any = [](bool q) { return __any(q) != 0; };
    double dd, l, xs[1][D];
    int st, rd;
    pairdist::iterate<D, 1>(
        v0, go, any,
        [&](const bool run, const double(&u)[4], double(&pn)[1][4], double(&wn)[4], double& lbv, int& lst) {
            double h;
            int s;
            pairdist::side_lp<D, RV>(pA, pbeta, np, m, xc, side ? 1.0 : -1.0, u, run, any, h, pn[0], s);
            const double ho = __shfl_xor(h, 1, 64);
            const int so = __shfl_xor(s, 1, 64);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const double po = k < D ? __shfl_xor(pn[0][k], 1, 64) : 0.0;
                wn[k] = side ? po - pn[0][k] : pn[0][k] - po;
            }
            lbv = side ? -ho - h : -h - ho;
            lst = side ? pairdist::lp_status(so, s) : pairdist::lp_status(s, so);
        },
        [&](const double(&q)[1][D], double(&xi)[D], double(&xj)[D], bool& f) {
#pragma unroll
            for (int k = 0; k < D; ++k) {
                const double o = __shfl_xor(q[0][k], 1, 64);
                xi[k] = side ? o : q[0][k];
                xj[k] = side ? q[0][k] : o;
            }
            f = f & (__shfl_xor((int)f, 1, 64) != 0);
        },
        [&](const double(&q)[1][D], const double tol) { return pairdist::inside_rows<D, RV>(pA, pbeta, np, q[0], xc, tol); }, dd, l,
        xs, st, rd);
    if (!listed) return;
    const double qnan = __builtin_nan("");
    if (side == 0) {
        dist[t] = go ? dd : qnan;
        status[t] = go ? st : pairdist::PAIR_BAD;
        if (lbout) lbout[t] = go ? l : qnan;
    }
    double* pout = side ? yout : xout;
    if (pout) {
#pragma unroll
        for (int k = 0; k < D; ++k) pout[t * D + k] = go ? xs[0][k] : qnan;
    }
}

// dist[K], lb[K], x[K][d], y[K][d] (each of the last three or nullptr), status[K] of plp_pair_dist; 0 when launched, 2 for a
// size the kernel does not take
int launch_pair_dist(int n, int m_max, int d, const double* A, const double* b, const int* mrows, const double* xc, long long K,
                     const int* pairs, double* dist, double* lb, double* x, double* y, int* status, hipStream_t st) {
    const int rv = rowtile::row_slots(m_max);
    if (n < 1 || K < 1 || K > 2147483647ll || rv == 0) return 2;
    const int np = rowtile::polytopes_per_group(1, rv);
    const long long blocks = (K + np / 2 - 1) / (np / 2);
    return rowtile::dispatch(d, rv, [&](auto dim, auto rows) {
        constexpr int D = decltype(dim)::value, RV = decltype(rows)::value;
        hipLaunchKernelGGL((pair_dist_kernel<D, RV>), dim3((unsigned)blocks), dim3(rowtile::BLOCK), rowtile::lds_bytes(D, RV, np, 1), st,
                           n, m_max, A, b, mrows, xc, K, pairs, np, dist, lb, x, y, status);
    });
}

}  // namespace plp
