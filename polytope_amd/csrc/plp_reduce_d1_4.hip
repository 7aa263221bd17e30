// plp_reduce_d1_4.hip -- the fused reduce's launches for d = 1..4 (plp_reduce_launch.hpp): instantiations only, one
// translation unit per range of d to keep the build parallel.  (PLP_STAGE_STATS builds: the counters of the bench shape's
// lane-group kernels, scripts/debug/stage_stats.sh)
#include "plp_reduce_launch.hpp"

namespace plp {

PLP_REDUCE_INSTANTIATE(1)
PLP_REDUCE_INSTANTIATE(2)
PLP_REDUCE_INSTANTIATE(3)
PLP_REDUCE_INSTANTIATE(4)

}  // namespace plp

#ifdef PLP_STAGE_STATS
extern "C" __attribute__((visibility("default"))) int plp_debug_stage_stats(unsigned long long* out16, int reset) {
    (void)hipDeviceSynchronize();
    if (out16 && hipMemcpyFromSymbol(out16, HIP_SYMBOL(plp::plp_stage_stats), 128) != hipSuccess) return 1;
    if (reset) {
        unsigned long long z[16] = {0};
        if (hipMemcpyToSymbol(HIP_SYMBOL(plp::plp_stage_stats), z, 128) != hipSuccess) return 1;
    }
    return 0;
}
#endif
