// plp_reduce_d13_16.hip -- the fused reduce's launches for d = 13..16 (plp_reduce_launch.hpp): instantiations only, one
// translation unit per range of d to keep the build parallel.
#include "plp_reduce_launch.hpp"

namespace plp {

PLP_REDUCE_INSTANTIATE(13)
PLP_REDUCE_INSTANTIATE(14)
PLP_REDUCE_INSTANTIATE(15)
PLP_REDUCE_INSTANTIATE(16)

}  // namespace plp
