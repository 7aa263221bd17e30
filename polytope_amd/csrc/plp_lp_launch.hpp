// plp_lp_launch.hpp -- the launchers that carry out one launch of a plan of plp_lp_plan.hpp, each in the translation unit
// of its kernels (internal to plp_lp.hip and those units).  No decisions here: the engine, the lanes per LP, the grid, the
// workgroup and the LDS bytes are the plan's.  Every launcher returns 0, or 2 for a shape its kernels do not exist for.
#pragma once
#include <type_traits>

#include "plp_kernels.hpp"
#include "plp_lp_plan.hpp"

namespace plp {

static_assert(LP_GENERAL_BLOCK == BLOCK && LP_MAX_M == MAX_M && LP_MAX_D == MAX_D, "the plan's envelope is plp_common.hpp's");

// the batch and the outputs of each call (BoxArgs::ho: nullptr where the caller takes nothing)
struct LpArgs { long long B; int m_max; const double *c, *G, *h; const int* mrows; double *x, *fun; int *status, *iters; };
struct ChebyArgs { long long B; int m_max; const double *A, *b; const int* mrows; double *r, *xc; int* status; };
struct BoxArgs { long long B; int m_max; const double *A, *b; const int* mrows; double *lb, *ub; int* status; BoxHandover ho; };
struct PairArgs {
    int n, m_max;
    const double *A, *b;
    const int* mrows;
    double inflate, thresh;
    unsigned char* adj;
    long long p_lo, p_hi;
    unsigned char* compact;
    int cross_n1;
    int mark;   // an LP that ends "unbounded" or at the iteration limit is written as PAIR_OPEN (the careful pass follows), not 0
    const int* list = nullptr;   // the listed form (plp_pair_list): p_hi pairs (list[2 t], list[2 t + 1]) into compact[t]
};

// f(std::integral_constant<int, K>()) for K == d in LO .. HI -> what f returns (0 when nothing); 2 when d is outside (the
// kernels exist for LO .. HI only)
template <class F, class K>
inline int call_with(F& f, K k) {
    if constexpr (std::is_void_v<decltype(f(k))>) {
        f(k);
        return 0;
    } else {
        return f(k);
    }
}
template <int LO, int HI, class F>
inline int for_dim(int d, F&& f) {
    if constexpr (LO > HI) {
        return 2;
    } else {
        return d == LO ? call_with(f, std::integral_constant<int, LO>()) : for_dim<LO + 1, HI>(d, f);
    }
}
// the same over the lanes per LP that exist at R rows per lane: 4, 8, 16, with fewer than four rows 32, with one 64
template <int R, class F>
inline int for_gs(int gs, F&& f) {
    if (gs == 4) return call_with(f, std::integral_constant<int, 4>());
    if (gs == 8) return call_with(f, std::integral_constant<int, 8>());
    if (gs == 16) return call_with(f, std::integral_constant<int, 16>());
    if constexpr (R < 4) {
        if (gs == 32) return call_with(f, std::integral_constant<int, 32>());
    }
    if constexpr (R < 2) {
        if (gs == 64) return call_with(f, std::integral_constant<int, 64>());
    }
    return 2;
}

// generic LPs: lp_r_kernel, then lp_p1_r_kernel when p1 is not null (plp_lp_r.hip); lp_w_kernel (plp_lp_wide.hip); lp_lds_kernel
int launch_lp_r(int n, const LpLaunch& L, const LpLaunch* p1, const LpArgs& a, hipStream_t st);
int launch_lp_w(int n, const LpLaunch& L, const LpArgs& a, hipStream_t st);
int launch_lp_lds(int n, const LpLaunch& L, const LpArgs& a, hipStream_t st);
// Chebyshev balls: cheby_r_kernel (plp_cheby_r.hip), cheby_w_kernel (plp_wide.hip), cheby_lds_kernel (plp_lds.hip)
int launch_cheby_r(int d, const LpLaunch& L, int force_retry, const ChebyArgs& a, hipStream_t st);
int launch_cheby_w(int d, const LpLaunch& L, const ChebyArgs& a, hipStream_t st);
int launch_cheby_lds(int d, const LpLaunch& L, const ChebyArgs& a, hipStream_t st);
// boxes: bbox_lane_kernel (plp_bbox_lane.hip), bbox_lazy_kernel / bbox_wsplit_kernel (plp_bbox_lazy.hip), bbox_r_kernel /
// bbox_split_kernel (plp_bbox_r.hip)
int launch_bbox_lane(int d, const LpLaunch& L, const BoxArgs& a, hipStream_t st);
int launch_bbox_lazy(int d, const LpLaunch& L, const BoxArgs& a, hipStream_t st);
int launch_bbox_r(int d, const LpLaunch& L, int force_retry, const BoxArgs& a, hipStream_t st);
// pairs: adjacent_r_kernel (plp_cheby_r.hip), adjacent_w_kernel (plp_wide.hip)
int launch_adjacent_r(int d, const LpLaunch& L, int force_retry, const PairArgs& a, hipStream_t st);
int launch_adjacent_w(int d, const LpLaunch& L, const PairArgs& a, hipStream_t st);
// ... and their listed instantiations, adjacent_r_list_kernel / adjacent_w_list_kernel
int launch_adjacent_r_list(int d, const LpLaunch& L, int force_retry, const PairArgs& a, hipStream_t st);
int launch_adjacent_w_list(int d, const LpLaunch& L, const PairArgs& a, hipStream_t st);

}  // namespace plp
