// plp_envelope.hip -- envelope_cross_kernel<D>: the facet tests of envelope() for many regions in one launch, one (region,
// member) list entry per wavefront (plp_envelope.hpp: the contract, the caps, the rule).  The owner's rows sit in LDS, a
// partner's rows are read from global memory once and stay in registers while every row of the owner that is still under
// test is stacked under them, and every Chebyshev LP runs on the one-LP-per-wavefront engine (plp_wide.hpp).
#include "plp_kernels.hpp"
#include "plp_envelope.hpp"
#include "plp_wide.hpp"

namespace plp {

namespace {

// what env::walk() asks of the wavefront: all members wave-uniform except prow / pb (lane r: row r of the partner)
template <int D>
struct WaveOracle {
    static constexpr int D1 = D + 1;
    const int lane;
    const long long lo;   // the list starts at mem_idx[lo]
    const int mc_max;
    const double* __restrict__ Ag;
    const double* __restrict__ bg;
    const int* __restrict__ mcg;
    const int* __restrict__ mem_idx;
    const double* own;    // LDS: the owner's rows [m_i][D + 1]
    wide::WideShared<D1>& sh;
    double prow[D], pb;
    int mj;

    __device__ __forceinline__ void partner(const long long j) {
        const long long c = mem_idx ? (long long)mem_idx[lo + j] : lo + j;
        mj = env::member_rows(mcg, mc_max, c);
#pragma unroll
        for (int k = 0; k < D; ++k) prow[k] = 0.0;
        pb = 0.0;
        if (lane < mj) {   // (only rows < mc[c] of a listed member are read)
            const long long g = c * mc_max + lane;
#pragma unroll
            for (int k = 0; k < D; ++k) prow[k] = Ag[g * D + k];
            pb = bg[g];
        }
    }
    __device__ __forceinline__ double radius(const int ii) {
        // lane mj takes the negated row ii of the owner (every lane reads the same LDS address: a broadcast)
        const bool neg = lane == mj;
        double a[D];
#pragma unroll
        for (int k = 0; k < D; ++k) a[k] = neg ? -own[ii * D1 + k] : prow[k];
        const double bi = neg ? -own[ii * D1 + D] : pb;
        return wide::cheby_radius_rows<D>(lane, mj + 1, lane <= mj, a, bi, sh);
    }
};

}  // namespace

// Workgroup (= wavefront) w, w + grid, ... takes list entry w.  The region of w is found by bisection of reg_off: the same
// scalar reads on every lane (wave-uniform), no owner[] array is passed.
//   check : the entry's own two offsets hold it and end inside mem_idx[L]; the lanes look at the listed members 64 at a time
//           (index inside the table, 1 .. 63 rows); one that fails makes the entry ENV_UNSUPPORTED and nothing is run
//   stage : lane r < m_i puts row r of the owner into LDS
//   walk  : env::walk() -- crossed and open masks in wave-uniform registers
//   write : lane 0 writes outer[w], status[w], nlp[w]; nobody else writes them
template <int D>
__global__ __launch_bounds__(64) void envelope_cross_kernel(const long long C, const int mc_max, const double* __restrict__ Ag,
                                                            const double* __restrict__ bg, const int* __restrict__ mcg,
                                                            const long long B, const int* __restrict__ reg_off, const long long L,
                                                            const int* __restrict__ mem_idx, const double abs_tol,
                                                            unsigned long long* __restrict__ outer, int* __restrict__ status,
                                                            int* __restrict__ nlp) {
    constexpr int D1 = D + 1;
    __shared__ double own[env::MAX_LIST * D1];
    __shared__ wide::WideShared<D1> sh;
    const int lane = threadIdx.x;
    for (long long w = blockIdx.x; w < L; w += gridDim.x) {
        __syncthreads();   // (the last entry's reads of `own` are done)
        long long lo = 0, hi = 0;
        bool ok = env::list_bounds(reg_off, env::find_region(reg_off, B, w), w, L, lo, hi);
        if (ok) {
            bool bad = false;
            for (long long k = lo + lane; k < hi; k += 64) {
                const long long c = mem_idx ? (long long)mem_idx[k] : k;
                bad = bad || !env::member_ok(c, C, mcg, mc_max);
            }
            ok = __ballot(bad) == 0ull;
        }
        if (!ok) {
            if (lane == 0) {
                outer[w] = 0ull;
                status[w] = env::ENV_UNSUPPORTED;
                nlp[w] = 0;
            }
            continue;
        }
        const long long i = mem_idx ? (long long)mem_idx[w] : w;
        const int mi = env::member_rows(mcg, mc_max, i);
        if (lane < mi) {
            const long long g = i * mc_max + lane;
#pragma unroll
            for (int k = 0; k < D; ++k) own[lane * D1 + k] = Ag[g * D + k];
            own[lane * D1 + D] = bg[g];
        }
        __syncthreads();
        env::Walk s;
        env::begin(s, mi);
        WaveOracle<D> o{lane, lo, mc_max, Ag, bg, mcg, mem_idx, own, sh, {}, 0.0, 0};
        env::walk(s, hi - lo, w - lo, abs_tol, o);
        unsigned long long out;
        const int st = env::finish(s, out);
        if (lane == 0) {
            outer[w] = out;
            status[w] = st;
            nlp[w] = s.nlp;
        }
    }
}

// 0 when launched, 2 for a size the kernel does not take
int launch_envelope_cross(long long C, int mc_max, int d, const double* A, const double* b, const int* mc, long long B,
                          const int* reg_off, long long L, const int* mem_idx, double abs_tol, unsigned long long* outer,
                          int* status, int* nlp, hipStream_t st) {
    if (L < 1 || L > 2147483647ll || B < 1 || B > 2147483647ll || C < 0 || mc_max < 0) return 2;
    if (d < 1 || d > env::MAX_DIM) return 2;
    // a fixed grid striding over L: enough workgroups of one wavefront to fill the device several times over
    const long long cap = 1ll << 16;
    const unsigned grid = (unsigned)(L < cap ? L : cap);
#define PLP_ENV(K)                                                                                                           \
    case K:                                                                                                                  \
        hipLaunchKernelGGL((envelope_cross_kernel<K>), dim3(grid), dim3(64), 0, st, C, mc_max, A, b, mc, B, reg_off, L, mem_idx, \
                           abs_tol, outer, status, nlp);                                                                     \
        return 0;
    switch (d) {
        PLP_ENV(1) PLP_ENV(2) PLP_ENV(3) PLP_ENV(4) PLP_ENV(5) PLP_ENV(6) PLP_ENV(7) PLP_ENV(8)
        default: return 2;
    }
#undef PLP_ENV
}

}  // namespace plp
