// plp_reduce_launch.hpp -- carries out one launch of a reduce plan (plp_reduce_plan.hpp): the engine's kernel for dimension
// D with the plan's grid, workgroup and LDS.  No decisions here.  Instantiated per range of d in plp_reduce_d*.hip (separate
// translation units only to keep the build parallel); the templates each engine exists for are those named below.
#pragma once
#include "plp_reduce_general.hpp"
#include "plp_reduce_lane.hpp"
#include "plp_reduce_plan.hpp"
#include "plp_reduce_r_impl.hpp"

namespace plp {

static_assert(REDUCE_GENERAL_BLOCK == BLOCK, "workgroup of the general kernel");

// the arguments of every kernel on the lane-group engines
#define PLP_REDUCE_GO(KERNEL)                                                                                                   \
    hipLaunchKernelGGL(KERNEL, dim3((unsigned)L.grid), dim3(L.block), L.lds, st, a.B, a.m_max, a.A, a.b, a.mrows, a.abs_tol, \
                       force, a.keep, a.flags, a.r, a.xc, a.nlp, a.ctr, a.retry_word, a.epoch)

template <int D, int GS, int R>
static inline void reduce_go_group(const ReduceLaunch& L, const ReduceArgs& a, int force, hipStream_t st) {
    if (L.lds > 48 * 1024)  // 64 rows x d>=5: up to 82 KB of the CU's 160 KB
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(reduce_r_kernel<D, GS, R>),
                                  hipFuncAttributeMaxDynamicSharedMemorySize, (int)L.lds);
    PLP_REDUCE_GO((reduce_r_kernel<D, GS, R>));
}

#define PLP_REDUCE_GO_LANE(KERNEL)                                                                                              \
    hipLaunchKernelGGL(KERNEL, dim3((unsigned)L.grid), dim3(L.block), L.lds, st, a.B, a.m_max, a.A, a.b, a.mrows, a.abs_tol, \
                       force, a.keep, a.flags, a.r, a.xc, a.nlp, a.ctr)

// one launch of the plan; retry_only: the general kernel's second pass (RE_GENERAL only)
template <int D>
int launch_reduce_d(const ReduceLaunch& L, const ReduceArgs& a, int force, int retry_only, hipStream_t st) {
    static_assert(sizeof(wide::WideShared<D + 1>) == wide_shared_bytes(D), "plan's LDS of the one-LP-per-wavefront engines");
    static_assert(reduce_lazy_smem_bytes(D) == reduce_r_smem_bytes(64, D, 1) + lazy::lds_bytes<D>(), "lazy LDS");
    switch (L.engine) {
        case RE_GENERAL:
            hipLaunchKernelGGL(reduce_kernel<D>, dim3((unsigned)L.grid), dim3(L.block), L.lds, st, a.B, a.m_max, L.gs, a.A, a.b,
                               a.mrows, a.abs_tol, retry_only, a.keep, a.flags, a.r, a.xc, a.nlp,
                               retry_only ? a.retry_word : nullptr, a.epoch);
            return 0;
        case RE_LANE:
            if constexpr (D <= 4) {
                if (L.rows == 32) {
                    if (L.gs == 16) PLP_REDUCE_GO_LANE((reduce_lane_kernel<D, 16, 32>));
                    else PLP_REDUCE_GO_LANE((reduce_lane_kernel<D, 8, 32>));
                } else if (L.gs == 16) PLP_REDUCE_GO_LANE((reduce_lane_kernel<D, 16, 16>));
                else if (L.gs == 8) PLP_REDUCE_GO_LANE((reduce_lane_kernel<D, 8, 16>));
                else PLP_REDUCE_GO_LANE((reduce_lane_kernel<D, 4, 16>));
                return 0;
            }
            return 2;
        case RE_LANE_MIX:
            if constexpr (D <= 4) {
                if (L.rows == 32)
                    hipLaunchKernelGGL((reduce_lane_mix_kernel<D, 32, 8, 16>), dim3((unsigned)L.grid), dim3(L.block), L.lds, st,
                                       (int)L.nbig, a.B, a.m_max, a.A, a.b, a.mrows, a.abs_tol, force, a.keep, a.flags, a.r, a.xc,
                                       a.nlp, a.ctr);
                else
                    hipLaunchKernelGGL((reduce_lane_mix_kernel<D, 16, 4, 8>), dim3((unsigned)L.grid), dim3(L.block), L.lds, st,
                                       (int)L.nbig, a.B, a.m_max, a.A, a.b, a.mrows, a.abs_tol, force, a.keep, a.flags, a.r, a.xc,
                                       a.nlp, a.ctr);
                return 0;
            }
            return 2;
        case RE_GROUP:
            if constexpr (D <= 8) {
                if (L.rows == 4) {
                    if (L.gs == 4) reduce_go_group<D, 4, 4>(L, a, force, st);
                    else if (L.gs == 8) reduce_go_group<D, 8, 4>(L, a, force, st);
                    else reduce_go_group<D, 16, 4>(L, a, force, st);
                    return 0;
                }
                if constexpr (D >= 5) {
                    if (L.gs == 8) reduce_go_group<D, 8, 2>(L, a, force, st);
                    else if (L.gs == 16) reduce_go_group<D, 16, 2>(L, a, force, st);
                    else reduce_go_group<D, 32, 2>(L, a, force, st);
                    return 0;
                }
            } else {
                if (L.rows == 1) reduce_go_group<D, 64, 1>(L, a, force, st);
                else if (L.gs == 16) reduce_go_group<D, 16, 2>(L, a, force, st);
                else reduce_go_group<D, 32, 2>(L, a, force, st);
                return 0;
            }
            return 2;
        case RE_GROUP_MIX:
            if constexpr (D <= 4) {
                hipLaunchKernelGGL((reduce_r_mix_kernel<D>), dim3((unsigned)L.grid), dim3(L.block), L.lds, st, (int)L.nbig, a.B,
                                   a.m_max, a.A, a.b, a.mrows, a.abs_tol, force, a.keep, a.flags, a.r, a.xc, a.nlp, a.ctr,
                                   a.retry_word, a.epoch);
                return 0;
            }
            return 2;
        case RE_SPLIT:
            if constexpr (D <= 8) {
                if (L.gs == 4) PLP_REDUCE_GO((reduce_split_kernel<D, 4, 4>));
                else if (L.gs == 8) PLP_REDUCE_GO((reduce_split_kernel<D, 8, 4>));
                else PLP_REDUCE_GO((reduce_split_kernel<D, 16, 4>));
            } else {
                if (L.gs == 16) PLP_REDUCE_GO((reduce_split_kernel<D, 16, 2>));
                else PLP_REDUCE_GO((reduce_split_kernel<D, 32, 2>));
            }
            return 0;
        case RE_WDENSE:
        case RE_LAZY:
        case RE_WSPLIT:
            if constexpr (D >= 5) {
                if (L.engine == RE_WDENSE) PLP_REDUCE_GO((reduce_wdense_kernel<D>));
                else if (L.engine == RE_LAZY) PLP_REDUCE_GO((reduce_lazy_kernel<D>));
                else if (L.nw == 4) PLP_REDUCE_GO((reduce_wsplit_kernel<D, 4, (D <= PLP_REDUCE_WDENSE_MAXD)>));
                else PLP_REDUCE_GO((reduce_wsplit_kernel<D, 2, (D <= PLP_REDUCE_WDENSE_MAXD)>));
                return 0;
            }
            return 2;
        default:
            return 2;
    }
}

#undef PLP_REDUCE_GO
#undef PLP_REDUCE_GO_LANE

#define PLP_REDUCE_INSTANTIATE(D) \
    template int launch_reduce_d<D>(const ReduceLaunch&, const ReduceArgs&, int, int, hipStream_t);

}  // namespace plp
