// plp_row_tile.hpp -- what the shared-row lane kernels share: support_kernel (plp_support.*) and nearest_kernel
// (plp_nearest.*) each solve K small problems per polytope for B polytopes, one problem per lane, the rows of a tile of NP
// polytopes staged ONCE into LDS for all of them ("the shared-row skeleton").  This header owns the tile
// rules, the LDS layout, the staging walk, the lane -> (polytope, item) mapping, the round loop and the D x RV dispatch; a
// kernel of the family supplies what one staged row is, a per-polytope prologue, and what one lane does with one item.
// The first part also compiles for the host (g++, tests/cabi/*_host.cpp export it to the tests); the second is __HIPCC__.
//
// Tiles.  One wavefront per workgroup.  L = min(64, next power of two >= K) lanes per polytope would put 64 / L polytopes
// on the wavefront; the rows of NP polytopes take NP * RV * (D + NS) * 8 bytes of LDS (NS scalars staged beside the D
// columns of a row: 1 for support, 2 for nearest), so NP is capped per RV (and L raised to 64 / NP, the extra lanes idle)
// at a footprint that leaves room for four workgroups on a CU's 160 KiB at NS = 1: np_cap below, the table of DESIGN.md
// 4.11a (K >= 33: one polytope per workgroup, 0.5 .. 3 KiB).  The K items of a polytope take ceil(K / L) rounds; the second
// grid index cuts them into K-chunks of `rounds` rounds each, the rows staged once per (tile, K-chunk).
// LDS layout: POLYTOPE-INTERLEAVED as in plp_reduce_lane.hpp -- column k of row i of the tile's polytope p at
// cols[(i * D + k) * NP + p], the D columns of all RV rows first, then the NS scalar planes, scalar t of row i at
// plane_t[i * NP + p].  The lanes of one polytope read one address (a broadcast); lanes of different polytopes read
// consecutive doubles: within a 32-lane half at most 32 of them, 256 bytes = every bank once.
#pragma once
#include <stddef.h>

#include "plp_enum.hpp"   // wenum::dim / dispatch_dim

namespace plp {
namespace rowtile {

constexpr int BLOCK = 64;   // one wavefront per workgroup
constexpr int MAX_ROWS = 64;

// row slots for polytopes of up to m_max rows (0: not taken)
constexpr int row_slots(int m_max) { return m_max < 0 || m_max > MAX_ROWS ? 0 : (m_max <= 16 ? 16 : (m_max <= 32 ? 32 : 64)); }
// polytopes per workgroup at most
constexpr int np_cap(int rv) { return 1024 / rv; }
// polytopes per workgroup for K items per polytope: 64 / L, capped; each gets 64 / NP lanes
constexpr int polytopes_per_group(int K, int rv) {
    int L = 1;
    while (L < BLOCK && L < K) L <<= 1;
    return BLOCK / L < np_cap(rv) ? BLOCK / L : np_cap(rv);
}
// rounds of one K-chunk for L lanes per polytope: k_rounds, more only where the second grid index would pass 65535;
// k_rounds = 0: one chunk of all ceil(K / L) rounds
constexpr int chunk_rounds(int K, int L, int k_rounds) {
    const long long rounds = ((long long)K + L - 1) / L;
    const long long need = k_rounds ? (rounds + 65534) / 65535 : rounds;
    return need > k_rounds ? (int)need : k_rounds;
}
constexpr size_t lds_bytes(int D, int rv, int np, int NS) { return (size_t)np * rv * (D + NS) * sizeof(double); }
// rows of a polytope in use: m[p] held to 0 .. m_max
constexpr int clamp_rows(int m, int m_max) { return m < 0 ? 0 : (m > m_max ? m_max : m); }

// the launch of B polytopes x K items at rv row slots: grid (blocks, chunks) of BLOCK lanes
struct Grid {
    int np, rounds;
    long long blocks, chunks;
    constexpr bool fits() const { return blocks <= 2147483647ll && chunks <= 65535; }
};
constexpr Grid grid(long long B, int K, int rv, int k_rounds) {
    const int np = polytopes_per_group(K, rv), L = BLOCK / np, rounds = chunk_rounds(K, L, k_rounds);
    const long long per = (long long)rounds * L;
    return Grid{np, rounds, (B + np - 1) / np, ((long long)K + per - 1) / per};
}

// f(dim<D>{}, rows<RV>{}) for d = D in 1 .. 4 and rv = RV, one of row_slots' 16, 32, 64 -> 0; 2 for any other d (f is not
// called)
template <int RV>
struct rows {
    static constexpr int value = RV;
};
template <class F>
inline int dispatch(const int d, const int rv, F&& f) {
    return wenum::dispatch_dim(d, [&](auto dim) {
        if (rv == 16) f(dim, rows<16>{});
        else if (rv == 32) f(dim, rows<32>{});
        else f(dim, rows<64>{});
    });
}

#if defined(__HIPCC__)
// the staged rows in dynamic LDS: cols [RV * D][np], then NS scalar planes [RV][np]
template <int D, int RV>
__device__ __forceinline__ double* plane(double* cols, const int np, const int t) {
    return cols + (size_t)RV * (D + t) * np;
}

// what a lane works on: polytope P (pv: one of the batch; the lanes past it keep P = the tile's first), its rows m, and
// item jl of every round
struct Lane {
    int p, jl, L, m;
    bool pv;
    long long P;
};

// Stages the tile of workgroup blockIdx.x and returns this lane's place in it.  Slot (row i, polytope p) by lane,
// consecutive lanes on consecutive polytopes (LDS stores without a bank conflict).  ROW(a, b_i, live, P, n, s): what goes
// into the slot, n[D] and s[NS]; a and b_i are zero for rows i >= m[p] and polytopes past the batch, which are never read
// from global memory.  Ends with the workgroup's barrier.
template <int D, int RV, int NS, class RowF>
__device__ __forceinline__ Lane stage(double* cols, const long long B, const int m_max, const double* __restrict__ Ag,
                                      const double* __restrict__ bg, const int* __restrict__ mrows, const int np, RowF ROW) {
    const int lane = threadIdx.x;
    const long long tile = (long long)blockIdx.x * np;   // first polytope of this workgroup
    const int ntile = (B - tile) < np ? (int)(B - tile) : np;
    for (int s = lane; s < RV * np; s += BLOCK) {
        const int p = s % np, i = s / np;
        const bool pv = p < ntile;
        const long long P = tile + (pv ? p : 0);
        const bool live = pv & (i < clamp_rows(mrows ? mrows[P] : m_max, m_max));
        double a[D], n[D], sc[NS];
        const double* src = Ag + (P * m_max + (live ? i : 0)) * D;
#pragma unroll
        for (int k = 0; k < D; ++k) a[k] = live ? src[k] : 0.0;
        const double bi = live ? bg[P * m_max + i] : 0.0;
        ROW(a, bi, live, P, n, sc);
#pragma unroll
        for (int k = 0; k < D; ++k) cols[(i * D + k) * np + p] = n[k];
#pragma unroll
        for (int t = 0; t < NS; ++t) plane<D, RV>(cols, np, t)[i * np + p] = sc[t];
    }
    __syncthreads();
    Lane ln;
    ln.L = BLOCK / np;
    ln.p = lane / ln.L;
    ln.jl = lane % ln.L;
    ln.pv = ln.p < ntile;
    ln.P = tile + (ln.pv ? ln.p : 0);
    ln.m = ln.pv ? clamp_rows(mrows ? mrows[ln.P] : m_max, m_max) : 0;
    return ln;
}

// The rounds of K-chunk blockIdx.y: BODY(go, j, q) on EVERY lane in every round -- go: the lane has item j of its polytope,
// q = P * K + j the problem's index in the [B][K] outputs; a lane without one (a polytope past the batch, j >= K) gets
// go = false with j = 0 (a body that votes across the wavefront needs it there; any other returns at once).
// j and q are formed as ints (two registers less across the body than the 64-bit sum with the chunk's first item): EVERY
// launcher of a kernel on this frame has to refuse B * K > 2^31 - 1, as launch_support and launch_nearest do.
template <class BodyF>
__device__ __forceinline__ void for_rounds(const Lane& ln, const int K, const int rounds, BodyF BODY) {
    const long long j0 = (long long)blockIdx.y * rounds * ln.L;
    for (int rd = 0; rd < rounds; ++rd) {
        const long long jw = j0 + (rd * ln.L + ln.jl);   // (rounds * L <= 2^31: the place within a chunk is an int)
        const bool go = ln.pv & (jw < K);
        const int j = go ? (int)jw : 0;
        const int q = (int)ln.P * K + j;
        BODY(go, (long long)j, (long long)q);
    }
}
#endif

}  // namespace rowtile
}  // namespace plp
