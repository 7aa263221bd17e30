// plp_bbox_lane.hip -- bounding boxes of polytopes with up to 32 rows in d <= 3 on the one-LP-per-lane engine
// (bbox_lane_kernel, plp_reduce_lane.hpp), with the tile shapes of the fused reduce (plan_bbox, plp_lp_plan.hpp).
#include "plp_lp_launch.hpp"
#include "plp_reduce_lane.hpp"

namespace plp {

static_assert(BBOX_LANE_MAXM == 2 * LN_ROWS, "the lane form's row slots");

// bbox_lane_kernel<d, L.gs, L.rows>: 64 / gs polytopes per wavefront, 16 or 32 row slots each; leaves the points the box LPs
// ended on for the verifier
int launch_bbox_lane(int d, const LpLaunch& L, const BoxArgs& a, hipStream_t st) {
    const int force = 0;   // (nothing to force: what this kernel does not settle goes back to the caller as status 1)
    return for_dim<1, BBOX_LANE_MAXD>(d, [&](auto K) {
        constexpr int D = decltype(K)::value;
#define PLP_BBL(GSV, RV)                                                                                                      \
    hipLaunchKernelGGL((bbox_lane_kernel<D, GSV, RV>), dim3((unsigned)L.grid), dim3(L.block), L.lds, st, a.B, a.m_max, a.A, a.b, \
                       a.mrows, force, a.lb, a.ub, a.status, a.ho.xfin)
        if (L.rows == 32) { if (L.gs == 16) PLP_BBL(16, 32); else PLP_BBL(8, 32); }
        else if (L.gs == 16) PLP_BBL(16, 16);
        else if (L.gs == 8) PLP_BBL(8, 16);
        else PLP_BBL(4, 16);
#undef PLP_BBL
    });
}

}  // namespace plp
