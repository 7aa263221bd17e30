// The fused reduce's plan (polytope_amd/csrc/plp_reduce_plan.hpp, a pure host header) behind a C ABI for
// tests/test_reduce_plan.py.  env: the twelve switches in the order of ReduceEnv, each a string or NULL (unset).
#include "../../polytope_amd/csrc/plp_reduce_plan.hpp"

static plp::ReduceEnv env_of(const char* const* env) {
    plp::ReduceEnv e;
    const char** f[] = {&e.lane, &e.lane_gs, &e.lane_mix, &e.retry_all, &e.one_row, &e.r1,
                        &e.r2,   &e.lazy,    &e.split,    &e.half,      &e.wsplit,  &e.wdense};
    for (int k = 0; k < 12; ++k) *f[k] = env[k];
    return e;
}

extern "C" void reduce_plan(long long B, int m_max, int d, const char* const* env, long long* out) {
    const plp::ReducePlan p = plp::plan_reduce(B, m_max, d, env_of(env));
    const plp::ReduceLaunch& L = p.first;
    const long long v[] = {L.engine, L.gs, L.rows, L.nw, L.dense, L.nbig, L.grid, L.block, (long long)L.lds,
                           p.second, p.force_retry, p.retry.gs, p.retry.grid, (long long)p.retry.lds};
    for (int k = 0; k < 14; ++k) out[k] = v[k];
}

// The batch sizes at which the header's thresholds sit (tests/instance_cases.py asks the plan at each of them and at the
// next one): every PLP_REDUCE_*MAXB / *MINB macro, and the tile counts of the mixed launches as members (the tiles hold
// 16 / 8 / 4 / 2 polytopes).  -> how many were written (at most cap)
extern "C" int reduce_plan_thresholds(long long* out, int cap) {
    const long long v[] = {
        PLP_REDUCE_WG_MAXB, PLP_REDUCE_LANE_MINB, PLP_REDUCE_LANE4_MINB, PLP_REDUCE_LANE4_MINB_ROWS14,
        PLP_REDUCE_LANE32_GS16_MAXB, PLP_REDUCE_LANE_GS8_MAXB, PLP_REDUCE_LANE_GS16_MAXB,
        PLP_REDUCE_LANE_MIX_MINBLOCKS * 16ll, PLP_REDUCE_LANE_MIX_MINBLOCKS * 8ll, PLP_REDUCE_LANE_MIX_MINBLOCKS * 4ll,
        PLP_REDUCE_MIX_MINBLOCKS * 16ll, PLP_REDUCE_HALF_MAXBLOCKS * 16ll, PLP_REDUCE_HALF_MAXBLOCKS * 32ll,
        PLP_REDUCE_WS2_MAXB_DENSE, PLP_REDUCE_WS4_MAXB_DENSE8, PLP_REDUCE_WS4_MAXB_DENSE, PLP_REDUCE_WS2_MAXB_LAZY,
        PLP_REDUCE_WS4_MAXB_LAZY};
    int n = 0;
    for (long long x : v)
        if (n < cap) out[n++] = x;
    for (int d = 1; d <= 16; ++d)
        for (int gs = 4; gs <= 32; gs *= 2)
            if (n < cap) out[n++] = PLP_REDUCE_SPLIT_MAXB(d, gs);
    return n;
}

// The plan at every (d, m_max, B) of three lists under one set of switches: per launch of a plan -- the first, then the
// general kernel's second pass where one follows -- a record of nine numbers d, m_max, B, position, engine, gs, rows, nw,
// dense.  Unsupported sizes give no record.  -> records written (out holds 2 * nd * nm * nB of them)
extern "C" long long reduce_plan_sweep(const char* const* env, const int* ds, int nd, const int* ms, int nm,
                                       const long long* Bs, int nB, long long* out) {
    const plp::ReduceEnv e = env_of(env);
    long long n = 0;
    for (int i = 0; i < nd; ++i)
        for (int j = 0; j < nm; ++j)
            for (int k = 0; k < nB; ++k) {
                const plp::ReducePlan p = plp::plan_reduce(Bs[k], ms[j], ds[i], e);
                if (p.first.engine == plp::RE_NONE) continue;
                for (int pos = 0; pos < (p.second ? 2 : 1); ++pos) {
                    const plp::ReduceLaunch& L = pos ? p.retry : p.first;
                    const long long v[] = {ds[i], ms[j], Bs[k], pos, L.engine, L.gs, L.rows, L.nw, L.dense};
                    for (long long x : v) out[n++] = x;
                }
            }
    return n / 9;
}
