// plp_hull_enum.hip -- hull_enum_kernel<D>: the facets of B small point sets by enumeration of hyperplanes, one point set
// per wavefront (plp_hull_enum.hpp: the contract, the tolerances, the sequential rule this kernel reproduces bit for bit).
#include "plp_kernels.hpp"
#include "plp_hull_enum.hpp"

namespace plp {

// Workgroup P takes point set P.  Lane i holds point i (wenum::Member); centre and scale come from wave reductions, the
// staged points are compacted into LDS in index order.  Then rounds of 64 candidates: lane l of round t unranks subset
// 64 t + l, builds its plane and tests it against every staged point (all lanes read the same LDS address: a broadcast).
// A lane that finds every point on its plane ends the enumeration for the whole set (FLAT); the facets of lanes behind it
// in the round are never looked at, as in the sequential rule.  The round's facets go through the greedy filter
// (wenum::wave_greedy_round: the rows of earlier rounds first, then lane order); Ao and bo hold (nu, off) on the STAGED
// points while the enumeration runs.  At the end bo goes to the caller's coordinates.
// Ao and bo are read back, so they are not __restrict__.
template <int D>
__global__ __launch_bounds__(wenum::BLOCK) void hull_enum_kernel(const int n_max, const double* __restrict__ Xg,
                                                                 const int* __restrict__ npts,
                                                                 const unsigned long long* __restrict__ keepg, const int f_max,
                                                                 double* Ao, double* bo, unsigned long long* __restrict__ on,
                                                                 int* __restrict__ count, int* __restrict__ basis,
                                                                 int* __restrict__ status) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    double* sq = reinterpret_cast<double*>(smem_raw);           // [n_max][D], the first n in use
    int* sidx = reinterpret_cast<int*>(sq + (size_t)n_max * D);   // [n_max]: the original index of a staged point
    wenum::Member me(n_max, npts, keepg);
    const int lane = me.lane;
    const long long P = me.P;
    // ---- stage
    const bool live = me.live;
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
        const double lo = wenum::wave_min(live ? p[k] : __builtin_inf());
        const double hi = wenum::wave_max(live ? p[k] : -__builtin_inf());
        c[k] = hullenum::centre(lo, hi);
    }
    const double s = wenum::wave_max(live ? hullenum::reach<D>(p, c) : 0.0);
    me.compact(live);
    const int n = me.n;
    const bool take = hullenum::stageable<D>(s, n);   // (uniform)
    if (take && live) {
#pragma unroll
        for (int k = 0; k < D; ++k) sq[me.pos * D + k] = (p[k] - c[k]) / s;
        sidx[me.pos] = lane;
    }
    __syncthreads();
    // ---- rounds of 64 candidates
    double* Ap = Ao + P * f_max * D;
    double* bp = bo + P * f_max;
    unsigned long long* op = on + P * f_max;
    int* basp = basis ? basis + P * f_max * D : nullptr;
    const int T = take ? wenum::candidates<D>(n) : 0;
    int cnt = 0;
    bool over = false, flat = false;
    for (int base = 0; base < T && !over; base += wenum::BLOCK) {
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
            wenum::unrank<D>(n, rank, idx);
            kind = hullenum::candidate<D>(sq, sidx, n, idx, nu, off, w);
        }
        const unsigned long long flatm = __ballot(kind == hullenum::CAND_FLAT);
        const int first_flat = flatm ? __ffsll((long long)flatm) - 1 : wenum::BLOCK;
        over = wenum::wave_greedy_round(
            lane, kind == hullenum::CAND_FACET && lane < first_flat, cnt, f_max,
            [&](const int q) {
                double a[D];
#pragma unroll
                for (int k = 0; k < D; ++k) a[k] = Ap[(long long)q * D + k];
                return hullenum::same<D>(nu, off, a, bp[q]);
            },
            [&](const int src) {
                double a[D];
#pragma unroll
                for (int k = 0; k < D; ++k) a[k] = __shfl(nu[k], src);
                return hullenum::same<D>(nu, off, a, __shfl(off, src));
            },
            [&](const int q) {
#pragma unroll
                for (int k = 0; k < D; ++k) {
                    Ap[(long long)q * D + k] = nu[k];
                    if (basp) basp[(long long)q * D + k] = sidx[idx[k]];
                }
                bp[q] = off;
                op[q] = w;
            });
        if (flatm && !over) {   // (uniform)
            flat = true;
            break;
        }
    }
    if (flat) cnt = 0;
    // ---- the rows in the caller's coordinates, the rest of the slots, the count and the status
    for (int q = lane; q < cnt; q += wenum::BLOCK) bp[q] = hullenum::unstage<D>(Ap + (long long)q * D, bp[q], c, s);
    wenum::fill_tail(lane, Ap, basp, (long long)cnt * D, (long long)f_max * D);
    wenum::fill_tail(lane, bp, nullptr, cnt, f_max);
    for (int q = cnt + lane; q < f_max; q += wenum::BLOCK) op[q] = 0ull;
    if (lane == 0) {
        count[P] = cnt;
        status[P] = cnt == 0 ? hullenum::HS_FLAT : (over ? hullenum::HS_OVERFLOW : hullenum::HS_OK);
    }
}

// Ao[B][f_max][d], bo[B][f_max], on[B][f_max], count[B], basis[B][f_max][d] (or nullptr), status[B] of plp_hull_batch; 0
// when launched, 2 for a size the kernel does not take
int launch_hull_enum(long long B, int n_max, int d, const double* X, const int* npts, const unsigned long long* keep, int f_max,
                     double* Ao, double* bo, unsigned long long* on, int* count, int* basis, int* status, hipStream_t st) {
    if (B < 1 || B > 2147483647ll || n_max < 0 || n_max > wenum::MAX_ITEMS || f_max < 1) return 2;
    return wenum::dispatch_dim(d, [&](auto dim) {
        constexpr int D = decltype(dim)::value;
        hipLaunchKernelGGL((hull_enum_kernel<D>), dim3((unsigned)B), dim3(wenum::BLOCK), hullenum::lds_bytes(D, n_max), st, n_max,
                           X, npts, keep, f_max, Ao, bo, on, count, basis, status);
    });
}

}  // namespace plp
