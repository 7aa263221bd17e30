// The plans of the stand-alone LP, Chebyshev, bounding-box and pair batches (polytope_amd/csrc/plp_lp_plan.hpp, a pure host
// header) behind a C ABI for tests/test_lp_plan.py.  call: 0 plan_lp(B, m_max, n), 1 plan_cheby(B, m_max, d), 2 plan_bbox(B,
// m_max, d), 3 plan_pairs(n, m_max, d, p_lo, p_hi, compact, cross_n1).  env: the thirteen switches in the order of LpEnv, each
// a string or NULL (unset).  out: the number of launches (-1: unsupported), three figures of the call (LP: the general
// kernel's retry pass follows; the others: force_retry, then the hand-over mode of the boxes or p_lo, p_hi of the pairs),
// then per launch engine, gs, rows, nw, dense, grid, block, LDS bytes.
// lp_plan_thresholds and lp_plan_sweep serve the census of tests/instance_cases.py.
#include "../../polytope_amd/csrc/plp_lp_plan.hpp"

static void put(long long*& o, const plp::LpLaunch& L) {
    const long long v[] = {L.engine, L.gs, L.rows, L.nw, L.dense, L.grid, L.block, (long long)L.lds};
    for (long long x : v) *o++ = x;
}

static plp::LpEnv env_of(const char* const* env) {
    plp::LpEnv e;
    const char** f[] = {&e.lds,        &e.lp_wide,   &e.lp_1row,     &e.cheby_wide,       &e.cheby_1row,  &e.retry_all, &e.bbox_lane,
                        &e.bbox_split, &e.bbox_wide, &e.bbox_wsplit, &e.bbox_wsplit_maxb, &e.bbox_wdense, &e.adj_wide};
    for (int k = 0; k < 13; ++k) *f[k] = env[k];
    return e;
}

// The sizes at which the header's thresholds for one call sit (tests/instance_cases.py asks the plan at each of them and at
// the next one): batch sizes; for the pair calls the largest number of cells whose n (n - 1) / 2 pairs stay within
// ADJ_WIDE_SMALL_PAIRS.  (The grid limit LP_MAX_GRID is not among them: no test poses 2^31 LPs.)  -> how many were written
extern "C" int lp_plan_thresholds(int call, long long* out, int cap) {
    long long v[8];
    int nv = 0;
    if (call == 1) v[nv++] = PLP_WIDE_SMALL_B;
    if (call == 2) {
        const long long w[] = {PLP_REDUCE_LANE32_GS16_MAXB, PLP_REDUCE_LANE_GS8_MAXB, PLP_REDUCE_LANE_GS16_MAXB, plp::BBOX_WIDE_MIN_B,
                               plp::BBOX_WIDE_SMALL_B,      PLP_BBOX_WSPLIT_MAXB,     plp::bbox_split_maxb(4),   plp::bbox_split_maxb(16)};
        for (long long x : w) v[nv++] = x;
    }
    if (call == 3) {
        long long n = 2;
        while ((n + 1) * n / 2 <= plp::ADJ_WIDE_SMALL_PAIRS) ++n;
        v[nv++] = n;
    }
    int n = 0;
    for (int k = 0; k < nv; ++k)
        if (n < cap) out[n++] = v[k];
    return n;
}

static void lp_plan_one(int call, const long long* a, const plp::LpEnv& e, long long* out);

// The plan of one call at every (d, m_max, B) of three lists under one set of switches (pairs: B cells, the matrix form):
// per launch a record of nine numbers d, m_max, B, position, engine, gs, rows, nw, dense.  Refused and empty sizes give no
// record.  -> records written (out holds 3 * nd * nm * nB of them)
extern "C" long long lp_plan_sweep(int call, const char* const* env, const int* ds, int nd, const int* ms, int nm,
                                   const long long* Bs, int nB, long long* out) {
    const plp::LpEnv e = env_of(env);
    long long n = 0, one[4 + 3 * 8];
    for (int i = 0; i < nd; ++i)
        for (int j = 0; j < nm; ++j)
            for (int k = 0; k < nB; ++k) {
                const long long a[7] = {Bs[k], ms[j], ds[i], 0, 0, 0, 0};
                lp_plan_one(call, a, e, one);
                for (int pos = 0; pos < one[0]; ++pos) {
                    const long long* L = one + 4 + 8 * pos;
                    const long long v[] = {ds[i], ms[j], Bs[k], pos, L[0], L[1], L[2], L[3], L[4]};
                    for (long long x : v) out[n++] = x;
                }
            }
    return n / 9;
}

extern "C" void lp_plan(int call, const long long* a, const char* const* env, long long* out) {
    lp_plan_one(call, a, env_of(env), out);
}

static void lp_plan_one(int call, const long long* a, const plp::LpEnv& e, long long* out) {
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
