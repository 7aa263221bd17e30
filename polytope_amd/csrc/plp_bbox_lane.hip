// plp_bbox_lane.hip -- bounding boxes of polytopes with up to 32 rows in d <= 3 on the one-LP-per-lane engine
// (bbox_lane_kernel, plp_reduce_lane.hpp), with the tile shapes of the fused reduce (plp_reduce_plan.hpp).
#include "plp_reduce_lane.hpp"

namespace plp {

template <int D>
static int launch_bbox_lane_d(long long B, int m_max, const double* A, const double* b, const int* mrows, double* lb, double* ub,
                              int* status, hipStream_t st, double* xfin) {
    if (B > 2147483647ll) return 1;
    const int force = 0;   // (nothing to force: what this kernel does not settle goes back to the caller as status 1)
    const bool wide = m_max > LN_ROWS;
    int gs = wide ? (B <= PLP_REDUCE_LANE32_GS16_MAXB ? 16 : 8) : (B <= PLP_REDUCE_LANE_GS16_MAXB ? 16 : (B <= PLP_REDUCE_LANE_GS8_MAXB ? 8 : 4));
    const long long ng = 64 / gs;
    long long blocks = (B + ng - 1) / ng;
    if (blocks < 1) blocks = 1;
#define PLP_BBL(GSV, RV)                                                                                                     \
    hipLaunchKernelGGL((bbox_lane_kernel<D, GSV, RV>), dim3((unsigned)blocks), dim3(RBLOCK), reduce_lane_smem_bytes(D, GSV, RV), st, B, \
                       m_max, A, b, mrows, force, lb, ub, status, xfin)
    if (wide) { if (gs == 16) PLP_BBL(16, 32); else PLP_BBL(8, 32); }
    else if (gs == 16) PLP_BBL(16, 16);
    else if (gs == 8) PLP_BBL(8, 16);
    else PLP_BBL(4, 16);
#undef PLP_BBL
    return 0;
}

// the contract of launch_bbox; 0 when launched, 1 when not taken
int launch_bbox_lane(long long B, int m_max, int d, const double* A, const double* b, const int* mrows, double* lb, double* ub,
                     int* status, hipStream_t st, double* xfin) {
    if (m_max < 1 || m_max > 2 * LN_ROWS) return 1;
    switch (d) {
        case 1: return launch_bbox_lane_d<1>(B, m_max, A, b, mrows, lb, ub, status, st, xfin);
        case 2: return launch_bbox_lane_d<2>(B, m_max, A, b, mrows, lb, ub, status, st, xfin);
        case 3: return launch_bbox_lane_d<3>(B, m_max, A, b, mrows, lb, ub, status, st, xfin);
        default: return 1;
    }
}

}  // namespace plp
