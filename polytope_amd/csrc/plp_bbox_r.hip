// plp_bbox_r.hip -- launcher of the fused bounding-box batches on the lane groups, d <= 8 (kernels: plp_cheby_r_impl.hpp).
#include "plp_cheby_r_impl.hpp"

namespace plp {

// LE_GROUP: bbox_r_kernel, 64 / gs polytopes per wavefront; LE_SPLIT: bbox_split_kernel, one polytope per wavefront, its 2d
// LPs over the lane groups.  Both leave the bases and the centres for the verifier.
int launch_bbox_r(int d, const LpLaunch& L, int force_retry, const BoxArgs& a, hipStream_t st) {
    return for_dim<1, 8>(d, [&](auto K) {
        constexpr int D = decltype(K)::value;
        return for_gs<RowsPerLane<D>::value>(L.gs, [&](auto G) {
            constexpr int GS = decltype(G)::value;
            if (L.engine == LE_SPLIT)
                hipLaunchKernelGGL((bbox_split_kernel<D, GS>), dim3((unsigned)L.grid), dim3(L.block), L.lds, st, a.B, a.m_max, a.A,
                                   a.b, a.mrows, a.lb, a.ub, a.status, force_retry, a.ho.basis8, a.ho.centre);
            else
                hipLaunchKernelGGL((bbox_r_kernel<D, GS>), dim3((unsigned)L.grid), dim3(L.block), L.lds, st, a.B, a.m_max, a.A,
                                   a.b, a.mrows, a.lb, a.ub, a.status, force_retry, a.ho.basis8, a.ho.centre);
        });
    });
}

}  // namespace plp
