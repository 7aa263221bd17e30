// plp_volume.hpp -- the arithmetic of the Monte-Carlo volume (reference: volume, polytope/polytope.py:1529-1594):
// numpy's PCG64 stream with exact jump-ahead, the sample in the bounding box, and the test of a sample against a
// polytope in contains_kernel's arithmetic (plp_points.hip).
//
// The generator.  np.random.default_rng(seed) is PCG64 (XSL-RR 128/64): a 128-bit LCG
//     state <- state * MULT + inc   (mod 2^128)
// whose output is rotr64(hi ^ lo, hi >> 58) of the NEW state, and a double is (u >> 11) * 2^-53.  Element (i, j) of
// random((n, N)) is stream position i * N + j, so it is pcg64_double(pcg64_out(state after i * N + j + 1 steps)).
// n steps of an LCG are one affine map  s -> A^n s + inc * G_n,  G_n = 1 + A + ... + A^(n - 1),  and neither A^n nor G_n
// depends on the stream: PCG64_POW holds the pairs (A^(2^k), G_(2^k)) for k < 64 (built at compile time from
// G_(2n) = G_n (1 + A^n)), pcg64_advance composes the pairs of the set bits of n -- O(popcount n) multiplications and no
// data-dependent squaring chain -- and pcg64_jump gives the pair of an arbitrary n for a caller that takes the same jump
// again and again (the kernel: by the workgroup's width from sample to sample, by N from coordinate to coordinate).
//
// 128-bit values are two uint64_t; products go through 32-bit limbs (no __int128: the same source is device code).
//
// The same source compiles for the device (plp_volume.hip) and for the host (tests/cabi/volume_host.cpp); both builds use
// -ffp-contract=off, so lb + r * w is a multiplication and an addition and the only fused operations are the fma() calls.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define PLP_VOL_FN __host__ __device__ __forceinline__ constexpr
#else
#define PLP_VOL_FN inline constexpr
#endif

namespace plp {
namespace vol {

struct u128 {
    uint64_t lo, hi;
};

constexpr u128 PCG64_MULT = {0x4385DF649FCCF645ull, 0x2360ED051FC65DA4ull};

// flags of plp_volume_hits: the polytope was not sampled (hits = 0)
enum : int { VF_NONFINITE = 1, VF_NOROWS = 2 };

// high 64 bits of a 64 x 64 product
PLP_VOL_FN uint64_t mul64_hi(uint64_t a, uint64_t b) {
    const uint64_t a0 = (uint32_t)a, a1 = a >> 32, b0 = (uint32_t)b, b1 = b >> 32;
    const uint64_t p00 = a0 * b0, p01 = a0 * b1, p10 = a1 * b0, p11 = a1 * b1;
    const uint64_t mid = (p00 >> 32) + (uint32_t)p01 + (uint32_t)p10;
    return p11 + (p01 >> 32) + (p10 >> 32) + (mid >> 32);
}

// a * b mod 2^128
PLP_VOL_FN u128 mul128_lo(u128 a, u128 b) {
    return u128{a.lo * b.lo, mul64_hi(a.lo, b.lo) + a.lo * b.hi + a.hi * b.lo};
}

PLP_VOL_FN u128 add128(u128 a, u128 b) {
    const uint64_t lo = a.lo + b.lo;
    return u128{lo, a.hi + b.hi + (lo < a.lo ? 1u : 0u)};
}

// a * x + c mod 2^128
PLP_VOL_FN u128 mad128(u128 a, u128 x, u128 c) { return add128(mul128_lo(a, x), c); }

PLP_VOL_FN u128 pcg64_step(u128 state, u128 inc) { return mad128(PCG64_MULT, state, inc); }

PLP_VOL_FN uint64_t pcg64_out(u128 state) {
    const uint64_t x = state.hi ^ state.lo;
    const unsigned r = (unsigned)(state.hi >> 58);
    return (x >> r) | (x << ((64u - r) & 63u));
}

PLP_VOL_FN double pcg64_double(uint64_t u) { return (double)(u >> 11) * (1.0 / 9007199254740992.0); }

// (A^(2^k), G_(2^k)), k < 64
struct PowTable {
    u128 a[64], g[64];
};
constexpr PowTable make_pow_table() {
    PowTable t{};
    u128 a = PCG64_MULT, g = u128{1, 0};
    for (int k = 0; k < 64; ++k) {
        t.a[k] = a;
        t.g[k] = g;
        g = mul128_lo(g, add128(a, u128{1, 0}));
        a = mul128_lo(a, a);
    }
    return t;
}
constexpr PowTable PCG64_POW = make_pow_table();

// the affine map of n steps: state -> a * state + inc * g
struct Jump {
    u128 a, g;
};
PLP_VOL_FN Jump pcg64_jump(uint64_t n) {
    Jump j{u128{1, 0}, u128{0, 0}};
    for (int k = 0; n; ++k, n >>= 1)
        if (n & 1u) {   // first j, then 2^k steps
            j.g = mad128(PCG64_POW.a[k], j.g, PCG64_POW.g[k]);
            j.a = mul128_lo(PCG64_POW.a[k], j.a);
        }
    return j;
}
PLP_VOL_FN u128 pcg64_apply(Jump j, u128 state, u128 inc) { return mad128(j.a, state, mul128_lo(inc, j.g)); }

// the state after n steps
PLP_VOL_FN u128 pcg64_advance(u128 state, u128 inc, uint64_t n) {
    for (int k = 0; n; ++k, n >>= 1)
        if (n & 1u) state = mad128(PCG64_POW.a[k], state, mul128_lo(inc, PCG64_POW.g[k]));
    return state;
}

// coordinate of a sample (ref :1586-1588: l_b + random * (u_b - l_b)); w = ub - lb
PLP_VOL_FN double sample_coord(double lb, double w, double r) { return lb + r * w; }

// one row against one sample, contains_kernel's arithmetic with abs_tol = 0 (ref :1589-1591: all(A x - b < 0))
template <int D>
#if defined(__HIPCC__)
__host__ __device__ __forceinline__
#else
inline
#endif
bool row_inside(const double* a, double bi, const double* x) {
    double s = a[0] * x[0];
#pragma unroll
    for (int k = 1; k < D; ++k) s = fma(a[k], x[k], s);
    return (s - bi) < 0.0;
}

}  // namespace vol
}  // namespace plp
