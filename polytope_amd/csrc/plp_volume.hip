// plp_volume.hip -- Monte-Carlo volume of a batch of packed polytopes (reference: volume, polytope/polytope.py:1529-1594):
// how many of the N uniform samples of each polytope's bounding box lie strictly inside it, with the samples numpy's
// default_rng(seed).random((d, N)) would draw, generated in registers (plp_volume.hpp: PCG64 with exact jump-ahead).
//
// Work item = (polytope, tile of samples): a workgroup of BLOCK lanes walks its tile BLOCK * PPL samples at a time, lane t
// owning samples j_lo + t, j_lo + t + BLOCK, ...  A lane keeps ONE 128-bit generator state, positioned at its current
// sample's coordinate 0 (stream position j); coordinate k is position k * N + j, reached by k jumps of N, and the next
// sample by one jump of BLOCK from the kept state: d multiply-adds mod 2^128 per sample, exactly as many as d states
// stepped side by side would take, in 8 VGPRs instead of 4 d.  The multipliers of both jumps are per-call constants
// (kernel arguments, SGPRs); their increments are inc * G, two wave-uniform products per polytope.  A lane's first
// position: the tile's start from the polytope's state by pcg64_advance (wave-uniform), then the set bits of the lane
// number (8 predicated multiply-adds).
//
// The polytope's rows are wave-uniform and come through the scalar cache as in contains_kernel, each a_ik feeding PPL FMA
// chains in that kernel's order (a_0 x_0, then fma(a_k, x_k, s)), inside iff (s - b_i) < 0 for every row.  Verdicts are
// wave-wide lane masks; a wavefront adds its popcount to hits[p] with one atomicAdd.
#include <stdlib.h>

#include "plp_volume.hpp"
#include "plp_common.hpp"
#include "plp_kernels.hpp"

namespace plp {
namespace {

using vol::u128;

// sizes and per-call constants; the arrays are kernel parameters of their own so that they can be __restrict__ (the row
// loads must be provably unaffected by the atomicAdd on hits[] to be scalar loads)
struct VolArgs {
    long long B;
    int m_max;
    unsigned N, tile, ntiles;
    vol::Jump jn, js;   // N steps, BLOCK steps
};

template <int D, int PPL>
__global__ __launch_bounds__(BLOCK) void volume_hits_kernel(VolArgs a, const double* __restrict__ A,
                                                            const double* __restrict__ b, const int* __restrict__ mrows,
                                                            const double* __restrict__ lb, const double* __restrict__ ub,
                                                            const unsigned long long* __restrict__ state,
                                                            const unsigned long long* __restrict__ inc_w,
                                                            unsigned* __restrict__ hits, int* __restrict__ flags) {
    static_assert(BLOCK == 256, "the lane's start is composed from the 8 bits of its number");
    const long long total = a.B * (long long)a.ntiles;
    const unsigned tid = threadIdx.x;
    for (long long w = blockIdx.x; w < total; w += gridDim.x) {
        const long long p = w / a.ntiles;
        const unsigned t = (unsigned)(w - p * a.ntiles);
        int m = mrows ? mrows[p] : a.m_max;
        m = m < 0 ? 0 : (m > a.m_max ? a.m_max : m);
        double lo[D], wd[D];
        bool finite = true;
#pragma unroll
        for (int k = 0; k < D; ++k) {
            const double l = lb[p * D + k], u = ub[p * D + k];
            lo[k] = l;
            wd[k] = u - l;
            finite = finite && isfinite(l) && isfinite(u);
        }
        if (!finite || m == 0) {   // not sampled: hits stays 0, the caller decides
            if (t == 0 && tid == 0) flags[p] = (finite ? 0 : vol::VF_NONFINITE) | (m == 0 ? vol::VF_NOROWS : 0);
            continue;
        }
        const u128 inc{inc_w[2 * p], inc_w[2 * p + 1]};
        const u128 cn = vol::mul128_lo(inc, a.jn.g), cs = vol::mul128_lo(inc, a.js.g);
        const unsigned j_lo = t * a.tile;
        const unsigned j_hi = (a.N - j_lo < a.tile) ? a.N : j_lo + a.tile;
        // numpy steps, then outputs: sample j's coordinate 0 is the output of the state after j + 1 steps
        u128 s = vol::pcg64_advance(u128{state[2 * p], state[2 * p + 1]}, inc, (uint64_t)j_lo + 1u);
#pragma unroll
        for (int k = 0; k < 8; ++k)   // BLOCK = 2^8 lanes
            if ((tid >> k) & 1u) s = vol::mad128(vol::PCG64_POW.a[k], s, vol::mul128_lo(inc, vol::PCG64_POW.g[k]));
        const double* Ap = A + (size_t)p * a.m_max * D;
        const double* bp = b + (size_t)p * a.m_max;
        unsigned cnt = 0;   // of this wavefront
        for (unsigned j0 = j_lo; j0 < j_hi; j0 += BLOCK * PPL) {
            double x[PPL][D];
            unsigned long long ok_m[PPL];
#pragma unroll
            for (int u = 0; u < PPL; ++u) {
                u128 c = s;
                x[u][0] = vol::sample_coord(lo[0], wd[0], vol::pcg64_double(vol::pcg64_out(c)));
#pragma unroll
                for (int k = 1; k < D; ++k) {
                    c = vol::mad128(a.jn.a, c, cn);
                    x[u][k] = vol::sample_coord(lo[k], wd[k], vol::pcg64_double(vol::pcg64_out(c)));
                }
                s = vol::mad128(a.js.a, s, cs);
                // (j_hi - j0 > u * BLOCK + tid without overflow: j_hi < 2^31)
                ok_m[u] = __ballot(j0 + (unsigned)u * BLOCK + tid < j_hi);
            }
            for (int i = 0; i < m; ++i) {   // rows are wave-uniform: scalar loads, SGPR operands
                double ar[D];
#pragma unroll
                for (int k = 0; k < D; ++k) ar[k] = Ap[i * D + k];
                const double bi = bp[i];
#pragma unroll
                for (int u = 0; u < PPL; ++u) ok_m[u] &= __ballot(vol::row_inside<D>(ar, bi, x[u]));
            }
#pragma unroll
            for (int u = 0; u < PPL; ++u) cnt += (unsigned)__popcll(ok_m[u]);
        }
        if ((tid & 63u) == 0 && cnt) atomicAdd(&hits[p], cnt);
    }
}

template <int D>
void launch_volume_d(VolArgs a, const double* A, const double* b, const int* mrows, const double* lb, const double* ub,
                     const unsigned long long* state, const unsigned long long* inc, unsigned* hits, int* flags,
                     hipStream_t st) {
    // samples per lane and pass: each row fetched through the scalar cache feeds PPL FMA chains; 2 PPL D VGPRs of samples
    constexpr int PPL = (D <= 8) ? 4 : 2;
    constexpr unsigned CHUNK = BLOCK * PPL;
    // enough work items to fill 256 CUs several times over when the batch alone does not: tiles are whole passes
    constexpr long long TARGET = 4096;
    const unsigned passes = (a.N + CHUNK - 1) / CHUNK;
    long long per = (TARGET + a.B - 1) / a.B;
    if (per > passes) per = passes;
    if (per < 1) per = 1;
    const unsigned tile_passes = (unsigned)((passes + per - 1) / per);
    a.tile = tile_passes * CHUNK;
    a.ntiles = (passes + tile_passes - 1) / tile_passes;
    const long long total = a.B * (long long)a.ntiles;
    // beyond the cap a workgroup takes several work items in turn (PLP_VOLUME_MAX_GRID: a lower cap, for the test of that loop)
    long long cap = 1ll << 22;
    if (const char* e = getenv("PLP_VOLUME_MAX_GRID")) {
        const long long v = atoll(e);
        if (v >= 1 && v < cap) cap = v;
    }
    const long long grid = total < cap ? total : cap;
    hipLaunchKernelGGL((volume_hits_kernel<D, PPL>), dim3((unsigned)grid), dim3(BLOCK), 0, st, a, A, b, mrows, lb, ub, state,
                       inc, hits, flags);
}

}  // namespace

int launch_volume_hits(long long B, int m_max, int d, const double* A, const double* b, const int* mrows, const double* lb,
                       const double* ub, const unsigned long long* state, const unsigned long long* inc, long long N,
                       unsigned* hits, int* flags, hipStream_t st) {
    if (d < 1 || d > MAX_D || m_max < 0 || m_max > MAX_M || B < 0 || N < 1 || N > 0x7fffffffll) return 2;
    if (B == 0) return 0;
    (void)hipMemsetAsync(hits, 0, (size_t)B * sizeof(unsigned), st);
    (void)hipMemsetAsync(flags, 0, (size_t)B * sizeof(int), st);
    VolArgs a{B, m_max, (unsigned)N, 0u, 0u, vol::pcg64_jump((uint64_t)N), vol::pcg64_jump((uint64_t)BLOCK)};
#define PLP_CASE_V(K) case K: launch_volume_d<K>(a, A, b, mrows, lb, ub, state, inc, hits, flags, st); break;
    switch (d) {
        PLP_CASE_V(1) PLP_CASE_V(2) PLP_CASE_V(3) PLP_CASE_V(4) PLP_CASE_V(5) PLP_CASE_V(6) PLP_CASE_V(7) PLP_CASE_V(8)
        PLP_CASE_V(9) PLP_CASE_V(10) PLP_CASE_V(11) PLP_CASE_V(12) PLP_CASE_V(13) PLP_CASE_V(14) PLP_CASE_V(15)
        PLP_CASE_V(16)
        default: return 2;
    }
#undef PLP_CASE_V
    return 0;
}

}  // namespace plp
