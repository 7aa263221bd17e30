// plp_cheby_r.hip -- launchers of the Chebyshev-ball and pair-adjacency batches on R rows per lane
// (kernels: plp_cheby_r_impl.hpp).
#include "plp_cheby_r_impl.hpp"

namespace plp {

int launch_cheby_r(int d, const LpLaunch& L, int force_retry, const ChebyArgs& a, hipStream_t st) {
    return for_dim<1, MAX_D>(d, [&](auto K) {
        constexpr int D = decltype(K)::value;
        return for_gs<RowsPerLane<D>::value>(L.gs, [&](auto G) {
            hipLaunchKernelGGL((cheby_r_kernel<D, decltype(G)::value>), dim3((unsigned)L.grid), dim3(L.block), L.lds, st, a.B,
                               a.m_max, a.A, a.b, a.mrows, a.r, a.xc, a.status, force_retry);
        });
    });
}

// d <= 8: the lane groups hold the stacked pair at four rows per lane only
int launch_adjacent_r(int d, const LpLaunch& L, int force_retry, const PairArgs& a, hipStream_t st) {
    return for_dim<1, 8>(d, [&](auto K) {
        constexpr int D = decltype(K)::value;
        return for_gs<RowsPerLane<D>::value>(L.gs, [&](auto G) {
            hipLaunchKernelGGL((adjacent_r_kernel<D, decltype(G)::value>), dim3((unsigned)L.grid), dim3(L.block), L.lds, st, a.n,
                               a.m_max, a.A, a.b, a.mrows, a.inflate, a.thresh, a.adj, a.p_lo, a.p_hi, a.compact, force_retry,
                               a.cross_n1, a.mark);
        });
    });
}

// the listed form (a.list, a.p_hi pairs into a.compact)
int launch_adjacent_r_list(int d, const LpLaunch& L, int force_retry, const PairArgs& a, hipStream_t st) {
    return for_dim<1, 8>(d, [&](auto K) {
        constexpr int D = decltype(K)::value;
        return for_gs<RowsPerLane<D>::value>(L.gs, [&](auto G) {
            hipLaunchKernelGGL((adjacent_r_list_kernel<D, decltype(G)::value>), dim3((unsigned)L.grid), dim3(L.block), L.lds, st,
                               a.n, a.m_max, a.A, a.b, a.mrows, a.inflate, a.thresh, a.p_hi, a.list, a.compact, force_retry, a.mark);
        });
    });
}

}  // namespace plp
