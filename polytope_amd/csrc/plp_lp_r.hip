// plp_lp_r.hip -- launcher of the generic LP batches on R rows per lane (kernels: plp_cheby_r_impl.hpp).
#include "plp_cheby_r_impl.hpp"

namespace plp {

// lp_r_kernel<n, L.gs>, then -- p1 not null, n = 3..PLP_P1_FAST_MAXN -- lp_p1_r_kernel on the same row slots
int launch_lp_r(int n, const LpLaunch& L, const LpLaunch* p1, const LpArgs& a, hipStream_t st) {
    return for_dim<1, MAX_D + 1>(n, [&](auto K) {
        constexpr int N = decltype(K)::value;
        return for_gs<RowsPerLane<N>::value>(L.gs, [&](auto G) {
            constexpr int GS = decltype(G)::value;
            hipLaunchKernelGGL((lp_r_kernel<N, GS>), dim3((unsigned)L.grid), dim3(L.block), L.lds, st, a.B, a.m_max, a.c, a.G, a.h,
                               a.mrows, a.x, a.fun, a.status, a.iters);
            if constexpr (P1_FAST<N>::value) {
                constexpr int RP = lp_p1_rows(N);
                if (p1)
                    hipLaunchKernelGGL((lp_p1_r_kernel<N, GS * RowsPerLane<N>::value / RP, RP>), dim3((unsigned)p1->grid),
                                       dim3(p1->block), p1->lds, st, a.B, a.m_max, a.c, a.G, a.h, a.mrows, a.x, a.fun, a.status,
                                       a.iters);
            }
        });
    });
}

}  // namespace plp
