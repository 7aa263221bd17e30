// The fused reduce's plan (polytope_amd/csrc/plp_reduce_plan.hpp, a pure host header) behind a C ABI for
// tests/test_reduce_plan.py.  env: the twelve switches in the order of ReduceEnv, each a string or NULL (unset).
#include "../../polytope_amd/csrc/plp_reduce_plan.hpp"

extern "C" void reduce_plan(long long B, int m_max, int d, const char* const* env, long long* out) {
    plp::ReduceEnv e;
    const char** f[] = {&e.lane, &e.lane_gs, &e.lane_mix, &e.retry_all, &e.one_row, &e.r1,
                        &e.r2,   &e.lazy,    &e.split,    &e.half,      &e.wsplit,  &e.wdense};
    for (int k = 0; k < 12; ++k) *f[k] = env[k];
    const plp::ReducePlan p = plp::plan_reduce(B, m_max, d, e);
    const plp::ReduceLaunch& L = p.first;
    const long long v[] = {L.engine, L.gs, L.rows, L.nw, L.dense, L.nbig, L.grid, L.block, (long long)L.lds,
                           p.second, p.force_retry, p.retry.gs, p.retry.grid, (long long)p.retry.lds};
    for (int k = 0; k < 14; ++k) out[k] = v[k];
}
