// The plans of the stand-alone LP, Chebyshev, bounding-box and pair batches (polytope_amd/csrc/plp_lp_plan.hpp, a pure host
// header) behind a C ABI for tests/test_lp_plan.py.  call: 0 plan_lp(B, m_max, n), 1 plan_cheby(B, m_max, d), 2 plan_bbox(B,
// m_max, d), 3 plan_pairs(n, m_max, d, p_lo, p_hi, compact, cross_n1).  env: the thirteen switches in the order of LpEnv, each
// a string or NULL (unset).  out: the number of launches (-1: unsupported), three figures of the call (LP: the general
// kernel's retry pass follows; the others: force_retry, then the hand-over mode of the boxes or p_lo, p_hi of the pairs),
// then per launch engine, gs, rows, nw, dense, grid, block, LDS bytes.
#include "../../polytope_amd/csrc/plp_lp_plan.hpp"

static void put(long long*& o, const plp::LpLaunch& L) {
    const long long v[] = {L.engine, L.gs, L.rows, L.nw, L.dense, L.grid, L.block, (long long)L.lds};
    for (long long x : v) *o++ = x;
}

extern "C" void lp_plan(int call, const long long* a, const char* const* env, long long* out) {
    plp::LpEnv e;
    const char** f[] = {&e.lds,        &e.lp_wide,   &e.lp_1row,     &e.cheby_wide,       &e.cheby_1row,  &e.retry_all, &e.bbox_lane,
                        &e.bbox_split, &e.bbox_wide, &e.bbox_wsplit, &e.bbox_wsplit_maxb, &e.bbox_wdense, &e.adj_wide};
    for (int k = 0; k < 13; ++k) *f[k] = env[k];
    long long* o = out + 4;
    plp::LpLaunch first;
    int n = 1;
    out[1] = out[2] = out[3] = 0;
    if (call == 0) {
        const plp::LpPlan p = plp::plan_lp(a[0], (int)a[1], (int)a[2], e);
        first = p.first;
        put(o, p.first);
        if (p.p1) { put(o, p.p1_launch); ++n; }
        if (p.second) { put(o, p.retry); ++n; }
        out[1] = p.second;
    } else if (call == 1) {
        const plp::ChebyPlan p = plp::plan_cheby(a[0], (int)a[1], (int)a[2], e);
        first = p.first;
        put(o, p.first);
        out[1] = p.force_retry;
    } else if (call == 2) {
        const plp::BoxPlan p = plp::plan_bbox(a[0], (int)a[1], (int)a[2], e);
        first = p.first;
        put(o, p.first);
        out[1] = p.force_retry;
        out[2] = p.handover;
    } else {
        const plp::PairPlan p = plp::plan_pairs((int)a[0], (int)a[1], (int)a[2], a[3], a[4], a[5] != 0, (int)a[6], e);
        first = p.first;
        put(o, p.first);
        out[1] = p.force_retry;
        out[2] = p.p_lo;
        out[3] = p.p_hi;
    }
    out[0] = first.engine == plp::LE_NONE ? -1 : (first.engine == plp::LE_EMPTY ? 0 : n);
}
