// plp_hull_enum.hip -- hull_enum_kernel<D>: the facets of B small point sets by enumeration of hyperplanes, one point set
// per wavefront (plp_hull_enum.hpp: the contract, the tolerances, the sequential rule this kernel reproduces bit for bit).
#include "plp_kernels.hpp"
#include "plp_hull_enum.hpp"

namespace plp {

constexpr int HS_BLOCK = 64;   // one wavefront per workgroup

// min / max over the wavefront (every lane gets the result; exact, so the order of the butterfly does not matter)
__device__ __forceinline__ double wave_min(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmin(v, __shfl_xor(v, o));
    return v;
}
__device__ __forceinline__ double wave_max(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o));
    return v;
}

// Workgroup P takes point set P.  Lane i holds point i (n_max <= 64: the points are read from memory once); centre and
// scale come from wave reductions, the staged points are compacted into LDS in index order.  Then rounds of 64
// candidates: lane l of round t unranks subset 64 t + l, builds its plane and tests it against every staged point (all
// lanes read the same LDS address: a broadcast).  A lane that finds every point on its plane ends the enumeration for the
// whole set (FLAT); the facets of lanes behind it in the round are never looked at, as in the sequential rule.  The greedy
// filter of a round: every facet lane first compares with the rows accepted in earlier rounds (read back from Ao and bo,
// which hold (nu, off) on the STAGED points while the enumeration runs and which this wavefront wrote: a workgroup barrier
// stands between the store and the load); the lanes that remain are resolved IN LANE ORDER -- the lowest one is accepted
// and broadcast, the others drop out if they are close to it -- because closeness is not transitive and the sequential
// rule compares a candidate with accepted rows only.  At the end bo goes to the caller's coordinates.
// Ao and bo are read back, so they are not __restrict__.
template <int D>
__global__ __launch_bounds__(HS_BLOCK) void hull_enum_kernel(const int n_max, const double* __restrict__ Xg,
                                                             const int* __restrict__ npts,
                                                             const unsigned long long* __restrict__ keepg, const int f_max,
                                                             double* Ao, double* bo, unsigned long long* __restrict__ on,
                                                             int* __restrict__ count, int* __restrict__ basis,
                                                             int* __restrict__ status) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    double* sq = reinterpret_cast<double*>(smem_raw);           // [n_max][D], the first n in use
    int* sidx = reinterpret_cast<int*>(sq + (size_t)n_max * D);   // [n_max]: the original index of a staged point
    const int lane = threadIdx.x;
    const long long P = blockIdx.x;
    int np_ = npts ? npts[P] : n_max;
    np_ = np_ < 0 ? 0 : (np_ > n_max ? n_max : np_);
    const unsigned long long keep = keepg ? keepg[P] : ~0ull;
    // ---- stage
    const bool live = lane < np_ && ((keep >> lane) & 1ull);
    double p[D], c[D];
#pragma unroll
    for (int k = 0; k < D; ++k) p[k] = 0.0;
    if (live) {
        const double* src = Xg + (P * n_max + lane) * D;
#pragma unroll
        for (int k = 0; k < D; ++k) p[k] = src[k];
    }
#pragma unroll
    for (int k = 0; k < D; ++k) {
        const double lo = wave_min(live ? p[k] : __builtin_inf());
        const double hi = wave_max(live ? p[k] : -__builtin_inf());
        c[k] = hullenum::centre(lo, hi);
    }
    const double s = wave_max(live ? hullenum::reach<D>(p, c) : 0.0);
    const unsigned long long livem = __ballot(live);
    const int n = __popcll(livem);
    const bool take = hullenum::stageable<D>(s, n);   // (uniform)
    if (take && live) {
        const int pos = __popcll(livem & ((1ull << lane) - 1ull));
#pragma unroll
        for (int k = 0; k < D; ++k) sq[pos * D + k] = (p[k] - c[k]) / s;
        sidx[pos] = lane;
    }
    __syncthreads();
    // ---- rounds of 64 candidates
    double* Ap = Ao + P * f_max * D;
    double* bp = bo + P * f_max;
    unsigned long long* op = on + P * f_max;
    int* basp = basis ? basis + P * f_max * D : nullptr;
    const int T = take ? extreme::candidates<D>(n) : 0;
    int cnt = 0;
    bool over = false, flat = false;
    for (int base = 0; base < T && !over; base += HS_BLOCK) {
        const int rank = base + lane;
        double nu[D], off = 0.0;
        int idx[D];
        uint64_t w = 0;
#pragma unroll
        for (int k = 0; k < D; ++k) {
            nu[k] = 0.0;
            idx[k] = 0;
        }
        int kind = hullenum::CAND_NONE;
        if (rank < T) {
            extreme::unrank<D>(n, rank, idx);
            kind = hullenum::candidate<D>(sq, sidx, n, idx, nu, off, w);
        }
        const unsigned long long flatm = __ballot(kind == hullenum::CAND_FLAT);
        const int first_flat = flatm ? __ffsll((long long)flatm) - 1 : HS_BLOCK;
        bool ok = kind == hullenum::CAND_FACET && lane < first_flat;
        if (__any(ok)) {
            for (int q = 0; q < cnt; ++q) {   // the rows of earlier rounds (every lane the same address)
                double a[D];
#pragma unroll
                for (int k = 0; k < D; ++k) a[k] = Ap[(long long)q * D + k];
                ok = ok && !hullenum::same<D>(nu, off, a, bp[q]);
            }
            unsigned long long rem = __ballot(ok);
            const bool wrote = rem != 0ull;
            while (rem) {   // this round's survivors, in lane order
                if (cnt == f_max) {
                    over = true;
                    break;
                }
                const int src = __ffsll((long long)rem) - 1;
                double a[D];
#pragma unroll
                for (int k = 0; k < D; ++k) a[k] = __shfl(nu[k], src);
                const double aoff = __shfl(off, src);
                if (lane == src) {
#pragma unroll
                    for (int k = 0; k < D; ++k) {
                        Ap[(long long)cnt * D + k] = nu[k];
                        if (basp) basp[(long long)cnt * D + k] = sidx[idx[k]];
                    }
                    bp[cnt] = off;
                    op[cnt] = w;
                    ok = false;
                } else if (ok && hullenum::same<D>(nu, off, a, aoff)) {
                    ok = false;
                }
                ++cnt;
                rem = __ballot(ok);
            }
            if (wrote) __syncthreads();   // (uniform: the next round, and the end, read what this one stored)
        }
        if (flatm && !over) {   // (uniform)
            flat = true;
            break;
        }
    }
    if (flat) cnt = 0;
    // ---- the rows in the caller's coordinates, the rest of the slots, the count and the status
    for (int q = lane; q < cnt; q += HS_BLOCK) bp[q] = hullenum::unstage<D>(Ap + (long long)q * D, bp[q], c, s);
    for (long long q = (long long)cnt * D + lane; q < (long long)f_max * D; q += HS_BLOCK) {
        Ap[q] = __builtin_nan("");
        if (basp) basp[q] = -1;
    }
    for (int q = cnt + lane; q < f_max; q += HS_BLOCK) {
        bp[q] = __builtin_nan("");
        op[q] = 0ull;
    }
    if (lane == 0) {
        count[P] = cnt;
        status[P] = cnt == 0 ? hullenum::HS_FLAT : (over ? hullenum::HS_OVERFLOW : hullenum::HS_OK);
    }
}

// Ao[B][f_max][d], bo[B][f_max], on[B][f_max], count[B], basis[B][f_max][d] (or nullptr), status[B] of plp_hull_batch; 0
// when launched, 2 for a size the kernel does not take
int launch_hull_enum(long long B, int n_max, int d, const double* X, const int* npts, const unsigned long long* keep, int f_max,
                     double* Ao, double* bo, unsigned long long* on, int* count, int* basis, int* status, hipStream_t st) {
    if (B < 1 || B > 2147483647ll || n_max < 0 || n_max > hullenum::MAX_POINTS || f_max < 1) return 2;
#define PLP_HS(D)                                                                                                         \
    hipLaunchKernelGGL((hull_enum_kernel<D>), dim3((unsigned)B), dim3(HS_BLOCK), hullenum::lds_bytes(D, n_max), st, n_max, X, \
                       npts, keep, f_max, Ao, bo, on, count, basis, status)
    switch (d) {
        case 1: PLP_HS(1); break;
        case 2: PLP_HS(2); break;
        case 3: PLP_HS(3); break;
        case 4: PLP_HS(4); break;
        default: return 2;
    }
#undef PLP_HS
    return 0;
}

}  // namespace plp
