// plp_reduce_d9_12.hip -- the fused reduce's launches for d = 9..12 (plp_reduce_launch.hpp): instantiations only, one
// translation unit per range of d to keep the build parallel.
#include "plp_reduce_launch.hpp"

namespace plp {

PLP_REDUCE_INSTANTIATE(9)
PLP_REDUCE_INSTANTIATE(10)
PLP_REDUCE_INSTANTIATE(11)
PLP_REDUCE_INSTANTIATE(12)

}  // namespace plp
