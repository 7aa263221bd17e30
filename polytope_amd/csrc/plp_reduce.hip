// plp_reduce.hip -- the fused reduce() of polytopes with up to 64 rows: plans the call (plp_reduce_plan.hpp) and carries
// the plan out (plp_reduce_launch.hpp, instantiated for every d in plp_reduce_d*.hip).
#include "plp_kernels.hpp"
#include "plp_reduce_plan.hpp"

namespace plp {

template <int D>
int launch_reduce_d(const ReduceLaunch& L, const ReduceArgs& a, int force, int retry_only, hipStream_t st);

static int launch_plan(int d, const ReduceLaunch& L, const ReduceArgs& a, int force, int retry_only, hipStream_t st) {
    switch (d) {
#define PLP_CASE_D(K) \
    case K: return launch_reduce_d<K>(L, a, force, retry_only, st);
        PLP_CASE_D(1) PLP_CASE_D(2) PLP_CASE_D(3) PLP_CASE_D(4) PLP_CASE_D(5) PLP_CASE_D(6) PLP_CASE_D(7) PLP_CASE_D(8)
        PLP_CASE_D(9) PLP_CASE_D(10) PLP_CASE_D(11) PLP_CASE_D(12) PLP_CASE_D(13) PLP_CASE_D(14) PLP_CASE_D(15) PLP_CASE_D(16)
#undef PLP_CASE_D
        default: return 2;
    }
}

int launch_reduce(int d, const ReduceArgs& a, int phase, hipStream_t st) {
    const ReducePlan p = plan_reduce(a.B, a.m_max, d, reduce_env());
    if (p.first.engine == RE_NONE) return 2;
    if (phase != 2) {
        const int rc = launch_plan(d, p.first, a, p.force_retry, 0, st);
        if (rc || !p.second || phase == 1) return rc;
    }
    return launch_plan(d, p.retry, a, p.force_retry, 1, st);
}

}  // namespace plp
