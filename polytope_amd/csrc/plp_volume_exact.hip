// plp_volume_exact.hip -- volume_exact_kernel<D>: the exact volumes and facet areas of B small polytopes by Lasserre's facet
// recursion on the rows, one polytope per wavefront (plp_volume_exact.hpp: the contract, the tolerances, the sequential
// rule this kernel reproduces bit for bit).
#include "plp_kernels.hpp"
#include "plp_volume_exact.hpp"

namespace plp {

// Workgroup P takes polytope P.  Lane i stages row i, the staged rows are compacted into LDS in row order (wenum::Member).
// The lanes then take the tuples of the last two chain levels, 64 to a round --
// (i1) at d = 2, (i1, i2) at d = 3, (i2, i3) under a wave-uniform loop over i1 at d = 4 -- and each evaluates its term
// (volume_exact::tuple_term: the chain's q, p and h in registers, one pass over the LDS rows in which every lane reads the
// same address, a broadcast) into the LDS term table.  The sums are the rule's: lane a adds row a of the table in index
// order (the stride is odd, so the lanes read different banks), at d = 4 weighs it and the facet's sum is taken over those
// in index order; the volume is the sum over the facets in index order, taken by every lane alike.  No atomics; every array
// in registers is indexed at compile time.
// At (64, 4) that is 64^3 tuples of 64 rows each per wavefront: milliseconds.  The cost grows as n^D.
template <int D>
__global__ __launch_bounds__(wenum::BLOCK) void volume_exact_kernel(const int m_max, const double* __restrict__ Ag,
                                                                const double* __restrict__ bg, const int* __restrict__ mrows,
                                                                const unsigned long long* __restrict__ keepg,
                                                                const double* __restrict__ xcg, const double* __restrict__ scaleg,
                                                                double* __restrict__ volume, double* __restrict__ area,
                                                                int* __restrict__ status) {
    using namespace volume_exact;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    double* sU = reinterpret_cast<double*>(smem_raw);   // [m_max][D], the first n in use
    double* sb = sU + (size_t)m_max * D;                // [m_max]
    double* fterm = sb + m_max;                         // [m_max]: the facets' terms (d = 2)
    double* fmeas = fterm + m_max;                      // [m_max]: the facets' measures
    double* tab = fmeas + m_max;                        // [n][tab_stride(n)] (d >= 3)
    wenum::Member me(m_max, mrows, keepg);
    const int lane = me.lane;
    const long long P = me.P;
    const double scale = scaleg ? scaleg[P] : 1.0;
    // ---- stage
    int kind = 0;
    double u[D], beta = 0.0;
#pragma unroll
    for (int k = 0; k < D; ++k) u[k] = 0.0;
    if (me.live) {
        double a[D], c[D];
        const double* src = Ag + (P * m_max + lane) * D;
#pragma unroll
        for (int k = 0; k < D; ++k) {
            a[k] = src[k];
            c[k] = xcg ? xcg[P * D + k] : 0.0;
        }
        kind = stage_row<D>(a, bg[P * m_max + lane], xcg != nullptr, c, scale, u, beta);
    }
    me.compact(kind == 1);
    const bool empty = __any(kind == 2) != 0;
    const int n = me.n, pos = me.pos;
    if (kind == 1) {
#pragma unroll
        for (int k = 0; k < D; ++k) sU[pos * D + k] = u[k];
        sb[pos] = beta;
    }
    __syncthreads();
    double* ap = area ? area + P * m_max : nullptr;
    if (empty) {   // (uniform)
        if (ap && lane < m_max) ap[lane] = 0.0;
        if (lane == 0) {
            volume[P] = 0.0;
            status[P] = VS_EMPTY;
        }
        return;
    }
    double vol = 0.0, mine = 0.0;   // mine: the area of this lane's row
    if (n == 0) {
        vol = inf();
    } else if constexpr (D == 1) {
        int own_lo, own_hi;
        vol = interval(sU, sb, n, own_lo, own_hi);
        mine = (kind == 1 && (pos == own_lo || pos == own_hi)) ? 1.0 : 0.0;
    } else if constexpr (D == 2) {
        if (lane < n) {
            const int idx[1] = {lane};
            double len;
            fterm[lane] = tuple_term<2>(sU, sb, n, idx, len);
            fmeas[lane] = len;
        }
        __syncthreads();
        for (int i1 = 0; i1 < n; ++i1) vol = vol + fterm[i1];
    } else {
        const int ns = tab_stride(n), T = n * n;
        const int outer = D == 4 ? n : 1;
        for (int o = 0; o < outer; ++o) {
            for (int base = 0; base < T; base += wenum::BLOCK) {
                const int rank = base + lane;
                if (rank < T) {
                    const int a = rank / n, c = rank - a * n;
                    int idx[Chain<D>::K];
                    double len;
                    if constexpr (D == 3) { idx[0] = a; idx[1] = c; } else { idx[0] = o; idx[1] = a; idx[2] = c; }
                    tab[a * ns + c] = tuple_term<D>(sU, sb, n, idx, len);
                }
            }
            __syncthreads();
            if (lane < n) {   // the table's rows
                double s = 0.0;
                for (int c = 0; c < n; ++c) s = s + tab[lane * ns + c];
                if constexpr (D == 3) {
                    fmeas[lane] = s;
                } else {
                    const int idx[Chain<D>::K] = {o, lane, 0};
                    tab[lane * ns] = weigh(prefix_h<D>(sU, sb, idx, 1), 3, s);
                }
            }
            __syncthreads();
            if constexpr (D == 4) {
                double s = 0.0;
                for (int a = 0; a < n; ++a) s = s + tab[a * ns];
                if (lane == 0) fmeas[o] = s;
                __syncthreads();   // (the next i1 writes the table again)
            }
        }
        for (int i1 = 0; i1 < n; ++i1) vol = vol + weigh(sb[i1], D, fmeas[i1]);
    }
    if (D > 1 && kind == 1) {
        const double f = fmeas[pos];
        mine = f == inf() ? f : power(scale, D - 1) * f;
    }
    if (ap && lane < m_max) ap[lane] = mine;
    if (lane == 0) {
        volume[P] = vol == inf() ? vol : power(scale, D) * vol;
        status[P] = vol == inf() ? VS_UNBOUNDED : VS_OK;
    }
}

// volume[B], area[B][m_max] (or nullptr), status[B] of plp_vol_exact_batch; 0 when launched, 2 for a size the kernel
// does not take
int launch_volume_exact(long long B, int m_max, int d, const double* A, const double* b, const int* mrows,
                        const unsigned long long* keep, const double* xc, const double* scale, double* volume, double* area,
                        int* status, hipStream_t st) {
    if (B < 1 || B > 2147483647ll || m_max < 0 || m_max > wenum::MAX_ITEMS) return 2;
    return wenum::dispatch_dim(d, [&](auto dim) {
        constexpr int D = decltype(dim)::value;
        hipLaunchKernelGGL((volume_exact_kernel<D>), dim3((unsigned)B), dim3(wenum::BLOCK), volume_exact::lds_bytes(D, m_max), st,
                           m_max, A, b, mrows, keep, xc, scale, volume, area, status);
    });
}

}  // namespace plp
