// plp_extreme.hip -- extreme_kernel<D>: the vertices of B small polytopes by enumeration of bases, one polytope per
// wavefront (plp_extreme.hpp: the contract, the tolerances, the sequential rule this kernel reproduces bit for bit).
#include "plp_kernels.hpp"
#include "plp_extreme.hpp"

namespace plp {

constexpr int XS_BLOCK = 64;   // one wavefront per workgroup

// Workgroup P takes polytope P.  Lane i stages row i (m_max <= 64: the rows are read from memory once), the staged rows
// are compacted into LDS in row order.  Then rounds of 64 candidates: lane l of round t unranks subset 64 t + l, solves it
// and tests it against every staged row (all lanes read the same LDS address: a broadcast).  The greedy filter of a round:
// every feasible lane first compares with the vertices accepted in earlier rounds (read back from V, which this
// wavefront wrote: a workgroup barrier stands between the store and the load); the lanes that remain are resolved IN LANE
// ORDER -- the lowest one is accepted and broadcast, the others drop out if they are close to it -- because closeness is
// not transitive and the sequential rule compares a candidate with accepted vertices only.
// V is read back, so it is not __restrict__.
template <int D>
__global__ __launch_bounds__(XS_BLOCK) void extreme_kernel(const int m_max, const double* __restrict__ Ag,
                                                           const double* __restrict__ bg, const int* __restrict__ mrows,
                                                           const unsigned long long* __restrict__ keepg, const int v_max,
                                                           double* V, int* __restrict__ basis, int* __restrict__ count,
                                                           int* __restrict__ status) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    double* sA = reinterpret_cast<double*>(smem_raw);   // [m_max][D], the first n in use
    double* sb = sA + (size_t)m_max * D;                // [m_max]
    int* sidx = reinterpret_cast<int*>(sb + m_max);     // [m_max]: the original index of a staged row
    const int lane = threadIdx.x;
    const long long P = blockIdx.x;
    int m = mrows ? mrows[P] : m_max;
    m = m < 0 ? 0 : (m > m_max ? m_max : m);
    const unsigned long long keep = keepg ? keepg[P] : ~0ull;
    // ---- stage
    int kind = 0;
    double u[D], beta = 0.0;
#pragma unroll
    for (int k = 0; k < D; ++k) u[k] = 0.0;
    if (lane < m && ((keep >> lane) & 1ull)) {
        double a[D];
        const double* src = Ag + (P * m_max + lane) * D;
#pragma unroll
        for (int k = 0; k < D; ++k) a[k] = src[k];
        kind = extreme::stage_row<D>(a, bg[P * m_max + lane], u, beta);
    }
    const unsigned long long staged = __ballot(kind == 1);
    const bool empty = __any(kind == 2) != 0;
    const int n = __popcll(staged);
    if (kind == 1) {
        const int pos = __popcll(staged & ((1ull << lane) - 1ull));
#pragma unroll
        for (int k = 0; k < D; ++k) sA[pos * D + k] = u[k];
        sb[pos] = beta;
        sidx[pos] = lane;
    }
    __syncthreads();
    // ---- rounds of 64 candidates
    double* Vp = V + P * v_max * D;
    int* bp = basis ? basis + P * v_max * D : nullptr;
    const int T = (!empty && n >= D) ? extreme::candidates<D>(n) : 0;
    int cnt = 0;
    bool over = false;
    for (int base = 0; base < T && !over; base += XS_BLOCK) {
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
            extreme::unrank<D>(n, rank, idx);
            ok = extreme::candidate<D>(sA, sb, n, idx, v);
        }
        if (!__any(ok)) continue;
        for (int q = 0; q < cnt; ++q) {   // the vertices of earlier rounds (every lane the same address)
            double w[D];
#pragma unroll
            for (int k = 0; k < D; ++k) w[k] = Vp[(long long)q * D + k];
            ok = ok && !extreme::same<D>(v, w);
        }
        unsigned long long rem = __ballot(ok);
        const bool wrote = rem != 0ull;
        while (rem) {   // this round's survivors, in lane order
            if (cnt == v_max) {
                over = true;
                break;
            }
            const int src = __ffsll((long long)rem) - 1;
            double w[D];
#pragma unroll
            for (int k = 0; k < D; ++k) w[k] = __shfl(v[k], src);
            if (lane == src) {
#pragma unroll
                for (int k = 0; k < D; ++k) {
                    Vp[(long long)cnt * D + k] = v[k];
                    if (bp) bp[(long long)cnt * D + k] = sidx[idx[k]];
                }
                ok = false;
            } else if (ok && extreme::same<D>(v, w)) {
                ok = false;
            }
            ++cnt;
            rem = __ballot(ok);
        }
        if (wrote) __syncthreads();   // (uniform: the next round reads what this one stored)
    }
    // ---- the rest of the slots, the count and the status
    for (long long q = (long long)cnt * D + lane; q < (long long)v_max * D; q += XS_BLOCK) {
        Vp[q] = __builtin_nan("");
        if (bp) bp[q] = -1;
    }
    if (lane == 0) {
        count[P] = cnt;
        status[P] = cnt == 0 ? extreme::XS_EMPTY : (over ? extreme::XS_OVERFLOW : extreme::XS_OK);
    }
}

// V[B][v_max][d], count[B], basis[B][v_max][d] (or nullptr), status[B] of plp_extreme_batch; 0 when launched, 2 for a size
// the kernel does not take
int launch_extreme(long long B, int m_max, int d, const double* A, const double* b, const int* mrows,
                   const unsigned long long* keep, int v_max, double* V, int* count, int* basis, int* status, hipStream_t st) {
    if (B < 1 || B > 2147483647ll || m_max < 0 || m_max > extreme::MAX_ROWS || v_max < 1) return 2;
#define PLP_XS(D)                                                                                                       \
    hipLaunchKernelGGL((extreme_kernel<D>), dim3((unsigned)B), dim3(XS_BLOCK), extreme::lds_bytes(D, m_max), st, m_max, A, b, \
                       mrows, keep, v_max, V, basis, count, status)
    switch (d) {
        case 1: PLP_XS(1); break;
        case 2: PLP_XS(2); break;
        case 3: PLP_XS(3); break;
        case 4: PLP_XS(4); break;
        default: return 2;
    }
#undef PLP_XS
    return 0;
}

}  // namespace plp
