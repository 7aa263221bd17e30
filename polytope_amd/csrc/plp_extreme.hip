// plp_extreme.hip -- extreme_kernel<D>: the vertices of B small polytopes by enumeration of bases, one polytope per
// wavefront (plp_extreme.hpp: the contract, the tolerances, the sequential rule this kernel reproduces bit for bit).
#include "plp_kernels.hpp"
#include "plp_extreme.hpp"

namespace plp {

// Workgroup P takes polytope P.  Lane i stages row i, the staged rows are compacted into LDS in row order (wenum::Member).
// Then rounds of 64 candidates: lane l of round t unranks subset 64 t + l, solves it and tests it against every staged
// row (all lanes read the same LDS address: a broadcast); the round's feasible candidates go through the greedy filter
// (wenum::wave_greedy_round: the vertices of earlier rounds first, then lane order).
// V is read back, so it is not __restrict__.
template <int D>
__global__ __launch_bounds__(wenum::BLOCK) void extreme_kernel(const int m_max, const double* __restrict__ Ag,
                                                               const double* __restrict__ bg, const int* __restrict__ mrows,
                                                               const unsigned long long* __restrict__ keepg, const int v_max,
                                                               double* V, int* __restrict__ basis, int* __restrict__ count,
                                                               int* __restrict__ status) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    double* sA = reinterpret_cast<double*>(smem_raw);   // [m_max][D], the first n in use
    double* sb = sA + (size_t)m_max * D;                // [m_max]
    int* sidx = reinterpret_cast<int*>(sb + m_max);     // [m_max]: the original index of a staged row
    wenum::Member me(m_max, mrows, keepg);
    const int lane = me.lane;
    const long long P = me.P;
    // ---- stage
    int kind = 0;
    double u[D], beta = 0.0;
#pragma unroll
    for (int k = 0; k < D; ++k) u[k] = 0.0;
    if (me.live) {
        double a[D];
        const double* src = Ag + (P * m_max + lane) * D;
#pragma unroll
        for (int k = 0; k < D; ++k) a[k] = src[k];
        kind = extreme::stage_row<D>(a, bg[P * m_max + lane], u, beta);
    }
    me.compact(kind == 1);
    const bool empty = __any(kind == 2) != 0;
    const int n = me.n;
    if (kind == 1) {
#pragma unroll
        for (int k = 0; k < D; ++k) sA[me.pos * D + k] = u[k];
        sb[me.pos] = beta;
        sidx[me.pos] = lane;
    }
    __syncthreads();
    // ---- rounds of 64 candidates
    double* Vp = V + P * v_max * D;
    int* bp = basis ? basis + P * v_max * D : nullptr;
    const int T = (!empty && n >= D) ? wenum::candidates<D>(n) : 0;
    int cnt = 0;
    bool over = false;
    for (int base = 0; base < T && !over; base += wenum::BLOCK) {
        const int rank = base + lane;
        double v[D];
        int idx[D];
#pragma unroll
        for (int k = 0; k < D; ++k) {
            v[k] = 0.0;
            idx[k] = 0;
        }
        bool ok = false;
        if (rank < T) {
            wenum::unrank<D>(n, rank, idx);
            ok = extreme::candidate<D>(sA, sb, n, idx, v);
        }
        over = wenum::wave_greedy_round(
            lane, ok, cnt, v_max,
            [&](const int q) {
                double w[D];
#pragma unroll
                for (int k = 0; k < D; ++k) w[k] = Vp[(long long)q * D + k];
                return extreme::same<D>(v, w);
            },
            [&](const int src) {
                double w[D];
#pragma unroll
                for (int k = 0; k < D; ++k) w[k] = __shfl(v[k], src);
                return extreme::same<D>(v, w);
            },
            [&](const int q) {
#pragma unroll
                for (int k = 0; k < D; ++k) {
                    Vp[(long long)q * D + k] = v[k];
                    if (bp) bp[(long long)q * D + k] = sidx[idx[k]];
                }
            });
    }
    // ---- the rest of the slots, the count and the status
    wenum::fill_tail(lane, Vp, bp, (long long)cnt * D, (long long)v_max * D);
    if (lane == 0) {
        count[P] = cnt;
        status[P] = cnt == 0 ? extreme::XS_EMPTY : (over ? extreme::XS_OVERFLOW : extreme::XS_OK);
    }
}

// V[B][v_max][d], count[B], basis[B][v_max][d] (or nullptr), status[B] of plp_extreme_batch; 0 when launched, 2 for a size
// the kernel does not take
int launch_extreme(long long B, int m_max, int d, const double* A, const double* b, const int* mrows,
                   const unsigned long long* keep, int v_max, double* V, int* count, int* basis, int* status, hipStream_t st) {
    if (B < 1 || B > 2147483647ll || m_max < 0 || m_max > wenum::MAX_ITEMS || v_max < 1) return 2;
    return wenum::dispatch_dim(d, [&](auto dim) {
        constexpr int D = decltype(dim)::value;
        hipLaunchKernelGGL((extreme_kernel<D>), dim3((unsigned)B), dim3(wenum::BLOCK), extreme::lds_bytes(D, m_max), st, m_max, A,
                           b, mrows, keep, v_max, V, basis, count, status);
    });
}

}  // namespace plp
