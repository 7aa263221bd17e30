// plp_reduce_d7_8.hip -- the fused reduce's launches for d = 7..8 (plp_reduce_launch.hpp): instantiations only, one
// translation unit per range of d to keep the build parallel.
#include "plp_reduce_launch.hpp"

namespace plp {

PLP_REDUCE_INSTANTIATE(7)
PLP_REDUCE_INSTANTIATE(8)

}  // namespace plp
