// plp_reduce_d5_6.hip -- the fused reduce's launches for d = 5..6 (plp_reduce_launch.hpp): instantiations only, one
// translation unit per range of d to keep the build parallel.
#include "plp_reduce_launch.hpp"

namespace plp {

PLP_REDUCE_INSTANTIATE(5)
PLP_REDUCE_INSTANTIATE(6)

}  // namespace plp
