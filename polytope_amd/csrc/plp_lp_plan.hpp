// plp_lp_plan.hpp -- which kernels the stand-alone LP, Chebyshev-ball, bounding-box and pair batches run, decided in one place.
//
// plan_lp / plan_cheby / plan_bbox / plan_pairs / plan_pair_list are pure host functions (no HIP): each names the engine,
// its tile shape, grid, workgroup and LDS bytes, and what follows the first launch.  The launchers (plp_lp.hip and the
// translation units of the kernels, plp_lp_launch.hpp) only carry the plan out.  tests/test_lp_plan.py pins it on the CPU
// (plan_pair_list: tests/test_box_pairs_host.py).
//
// The engines, by shape (defaults; rows = m_max, for pairs the stacked 2 m_max):
//   generic LPs   rows > 64      LDS: dictionary in LDS, one LP per wavefront (lp_lds_kernel), complete; NONE when the
//                                dictionary does not fit 160 KB
//                 n = 5..16      WIDE: one LP per wavefront, both phases (lp_w_kernel), complete
//                 other n <= 17  GROUP: four rows per lane (two from n = 9) on the origin-feasible LPs (lp_r_kernel), then
//                                lp_p1_r_kernel on those that need phase 1 (n = 3..PLP_P1_FAST_MAXN), then the general
//                                kernel's retry pass over what is still ST_RETRY (lp_kernel, retry_only)
//                 rows = 0, a grid beyond 2^31-1 workgroups: GENERAL, one row per lane (lp_kernel), alone
//   Chebyshev     rows > 64      LDS (cheby_lds_kernel)
//                 d >= 5 and (rows > 32 or B <= 4096): WIDE (cheby_w_kernel)
//                 else           GROUP, four / two rows per lane (cheby_r_kernel); GENERAL (cheby_kernel) as for LPs
//   boxes         d <= 3, rows <= 32: LANE, one LP per lane (bbox_lane_kernel), the tile shapes of the fused reduce
//                 d = 5..8 and (rows > 32 and B > 1024, or B <= 2000), d = 9..16: WIDE, one polytope per wavefront
//                                (bbox_lazy_kernel) or per workgroup of four (bbox_wsplit_kernel, B <= 2000), its 2d LPs
//                                with a stored dictionary up to d = 13
//                 else d <= 8    SPLIT, one polytope per wavefront over the lane groups (bbox_split_kernel), up to 4096
//                                polytopes (1024 at 16 lanes per polytope); GROUP (bbox_r_kernel) beyond
//   pairs         d > 8, d = 5..8 and (rows > 32 or at most 4096 pairs): WIDE (adjacent_w_kernel)
//                 else d <= 8    GROUP (adjacent_r_kernel)
// A/B switches (environment, read once per call by lp_env()).  "0/1": decided by the first character;
// "set": by being set at all, an empty value included.
//   PLP_LDS=1                the LDS engine for LPs and Chebyshev batches of any row count
//   PLP_LP_WIDE=0/1          n = 5..16: never / always WIDE; set with any other value: never
//   PLP_LP_1ROW=1            GENERAL alone (and no WIDE unless PLP_LP_WIDE=1)
//   PLP_CHEBY_WIDE=0/1       never / every d = 5..16 WIDE; set with any other value: never
//   PLP_CHEBY_1ROW=1         no GROUP: GENERAL where WIDE does not take the batch
//   PLP_CHEBY_RETRY_ALL=1    the lane-group kernels (Chebyshev, boxes, pairs, region_diff) hand every LP to their general engine
//   PLP_BBOX_LANE=0          no LANE
//   PLP_BBOX_SPLIT=0/1       lane groups: never / always SPLIT; set: no LANE, no small-batch WIDE
//   PLP_BBOX_WIDE=0/1        d = 5..8: never / always WIDE; set with any other value: never; set: no small-batch rule
//   PLP_BBOX_WSPLIT=0/1      WIDE: never / always four wavefronts per polytope; set: no small-batch WIDE at d = 5..8
//   PLP_BBOX_WSPLIT_MAXB=k   WIDE: four wavefronts per polytope up to k polytopes (a number, atoll)
//   PLP_BBOX_WDENSE=0/1      WIDE: the 2d LPs without / with a stored dictionary; set with any other value: without
//   PLP_ADJ_WIDE=0/1         d = 5..8: never / always WIDE (d > 8 is WIDE whatever it says); other values: never
#pragma once
#include <stddef.h>
#include <stdlib.h>

#include "plp_reduce_plan.hpp"  // the lane engine's tile shapes (PLP_REDUCE_LANE*_MAXB, reduce_lane_smem_bytes), RBLOCK

namespace plp {

// One wavefront per workgroup for the lane-group batch kernels (plp_cheby_r_impl.hpp; they use no LDS and no barrier): the
// tail of a launch is balanced wave by wave.  Against 256 threads (rocprofv3 kernel durations): lp_r_kernel<6,8> 271 -> 172 us,
// <16,32> 103 -> 81, <8,16> 186 -> 142, cheby_r_kernel<16,32> 692 -> 590, adjacent_r_kernel<4,4> 188 -> 181,
// lp_p1_r_kernel<3,4> 250 -> 199; cheby_r_kernel<3,4> and lp_r_kernel<3,4> at 100 k LPs unchanged.
#ifndef PLP_R_BLOCK
#define PLP_R_BLOCK 64
#endif
constexpr int RBLK = PLP_R_BLOCK;      // threads per workgroup of the lane-group kernels
constexpr int LP_GENERAL_BLOCK = 256;  // ... of lp_kernel / cheby_kernel (= BLOCK, plp_common.hpp)
constexpr int LP_MAX_M = 64;           // rows the register engines hold (= MAX_M)
constexpr int LP_MAX_D = 16;           // (= MAX_D; generic LPs: n <= LP_MAX_D + 1)
constexpr long long LP_MAX_GRID = 2147483647ll;  // workgroups of one launch

// ------------------------------------------------------------------------------------------- thresholds
// Chebyshev batches on the one-LP-per-wavefront engine (plp_wide.hip): d >= PLP_WIDE_MIN_D and either more than
// PLP_WIDE_MIN_M rows (the lane groups then hold one or two LPs per wavefront anyway and pay select chains for the
// entering column) or at most PLP_WIDE_SMALL_B LPs (every LP gets a wavefront slot at once: what counts is the latency
// of one LP, and a wave-uniform pivot is the shortest).  Measured with scripts/debug/wide_grid.py (round 3, after the
// pivot loop lost its register copies): (33..64 rows, d = 5..10) 15-40 % faster than the lane groups at B = 20 000,
// every shape with d >= 5 at B = 2 000; (<= 32 rows, B = 20 000) the lane groups stay 10-45 % ahead.
#ifndef PLP_WIDE_MIN_D
#define PLP_WIDE_MIN_D 5
#endif
#ifndef PLP_WIDE_MIN_M
#define PLP_WIDE_MIN_M 32
#endif
#ifndef PLP_WIDE_SMALL_B
#define PLP_WIDE_SMALL_B 4096
#endif
// The pair batches follow the same rule on the stacked pair, d = 5..8 (d > 8 has no lane-group kernel)
constexpr int ADJ_WIDE_MIN_ROWS = 32;
constexpr long long ADJ_WIDE_SMALL_PAIRS = 4096;

// Generic LP batches on the one-LP-per-wavefront engine (plp_lp_wide.hip): every batch with n = 5..16.  Measured against
// the lane-group kernels (scripts/debug/lp_wide_ab.py, 20 000 LPs, ms; x / status / iterations bitwise equal on every
// input): LPs that need phase 1 (64,16) 1.74 -> 0.34, (64,8) 0.59 -> 0.17, (32,12) 0.48 -> 0.17, (32,6) 0.21 -> 0.09,
// (16,5) 0.092 -> 0.063; origin-feasible ones (64,16) 0.43 -> 0.25, (32,6) a tie, (16,5) / (24,5) / (32,8) 10-30 % behind
// (four rows per lane pack several of those per wavefront) -- the mix of a batch is not known to the host, and the
// reference's LPs are posed in original coordinates, where the origin is rarely feasible.
// (A two-pass route for large batches of LPs with 32 rows and fewer -- lp_r_kernel for the origin-feasible ones, then this
// engine on what it hands over -- was measured: the feasible batches win their 15-27 % back, the two-phase ones lose
// 20-30 % to the extra pass ((32,6): 0.097 -> 0.116 ms); not kept.)

// Where the two-phase run on the fast path pays: measured on MI355X against the one-row-per-lane two-phase
// kernel (100k LPs, m=16): n=3 1.35x, n=4 1.22x, n=5 1.0x, n=6 0.88x, n=8 0.7x (the extra column, the carried
// cost row and the sign bookkeeping push four rows per lane past 250 VGPRs: one wave per SIMD), n=2 0.84x.
// Two rows per lane for n = 5..8 (groups twice as wide, two waves per SIMD) was measured too: 0.84x / 0.82x / 0.66x
// of the one-row kernel at (16,5) / (16,6) / (32,8) -- bitwise the same results, so the cut-off stays at n = 4.
#ifndef PLP_P1_FAST_MAXN
#define PLP_P1_FAST_MAXN 4
#endif

// Boxes, lane groups: the latency form (bbox_split_kernel, one polytope per wavefront, its 2d LPs over the lane groups) up
// to this many polytopes.  Measured device time per call, batch form: (16,3) B = 64 34 us, (32,6) 123 us, (64,8) 251 us.
// ((64,8) at B = 4096: 275 us batch form, 345 us latency form -- four groups per wavefront there)
constexpr long long bbox_split_maxb(int gs) { return gs >= 16 ? 1024 : 4096; }

// Boxes, d = 5..8 with more than 32 rows, beyond the latency form's batch sizes: one polytope per wavefront, wave-uniform
// pivots (plp_bbox_lazy.hip).  Measured (scripts/debug/bbox_wide_ab.py, ms): (64,8) B = 5 000 0.523 -> 0.262, B = 20 000
// 1.31 -> 0.82, (48,6) 0.52 -> 0.45, (33,5) 0.32 -> 0.30; the latency form keeps B <= 1024 ((64,8) B = 1000: 0.103
// against 0.157: its 2d LPs run side by side), the lane groups 32 rows and fewer ((32,6) 0.313 against 0.339).
// (round 4: and every batch of up to 2 000 polytopes, any row count: four wavefronts per polytope there, bbox_wsplit_kernel,
// 1.2x .. 1.85x ahead of the latency form; PLP_BBOX_SPLIT set: the lane-group forms keep their A/B meaning)
constexpr int BBOX_WIDE_MIN_M = 32;          // more rows than this ...
constexpr long long BBOX_WIDE_MIN_B = 1024;  // ... and more polytopes than this
constexpr long long BBOX_WIDE_SMALL_B = 2000;  // or at most this many polytopes
// Boxes, WIDE: four wavefronts per polytope up to this many polytopes.
// Measured (scripts/debug/bbox_wsplit_sweep.py, ms in use / four wavefronts per polytope): (64,8) B = 1 0.094 / 0.051, 500 0.116 /
// 0.071, 2 000 0.168 / 0.129; (32,6) 500 0.056 / 0.041; (64,12) 500 0.136 / 0.077, 2 000 0.168 / 0.151, 4 000 0.228 / 0.258;
// (64,16) 1 000 0.144 / 0.098
#ifndef PLP_BBOX_WSPLIT_MAXB
#define PLP_BBOX_WSPLIT_MAXB 2000
#endif
#ifndef PLP_BBOX_WDENSE_MAXD
#define PLP_BBOX_WDENSE_MAXD 13  // (as PLP_REDUCE_WDENSE_MAXD: beyond, the LPs are too short to pay for a dictionary reload)
#endif
// Boxes, LANE is d <= 3 only.  (d = 4 through walk4, measured and not enabled: 20-30 % ahead of the lane-group kernels from
// 2 000 polytopes on -- (16,4) x 100 000 209 -> 173 us, (32,4) 400 -> 290 -- but with no dedupe in front of it (bounding_box has
// none, ref :1314-1411) 20 of 6 407 polytopes with rows duplicated 1e-16 .. 1e-5 rad apart came out with a bound that is off
// by 2 (scripts/soak_lane.py 150 101, trial 97); the walk in R^3 hands such pairs back)
constexpr int BBOX_LANE_MAXD = 3;
constexpr int BBOX_LANE_MAXM = 32;

// ------------------------------------------------------------------------------------------- tile shapes, LDS, grids
// lanes per LP of the one-row-per-lane kernels for up to m_max rows (-1: unsupported)
constexpr int group_size_for(int m_max) {
    return (m_max < 0 || m_max > LP_MAX_M) ? -1 : (m_max <= 8 ? 8 : (m_max <= 16 ? 16 : (m_max <= 32 ? 32 : 64)));
}
// rows per lane of the lane-group kernels: 4 for d <= 8; 2 for d = 9..16, where four rows of up to 17 columns would not
// fit the VGPR file
#ifndef PLP_ROWS_BIG_D
#define PLP_ROWS_BIG_D 2
#endif
constexpr int lp_rows_per_lane(int d) { return d <= 8 ? 4 : PLP_ROWS_BIG_D; }
// lanes per LP for `rows` rows at R rows per lane: the smallest of 4 / 8 / 16 / 32 / 64 that holds them (0: none does)
constexpr int lp_group_size(int R, int rows) {
    return rows <= 4 * R ? 4 : (rows <= 8 * R ? 8 : (rows <= 16 * R ? 16 : ((R < 4 && rows <= 32 * R) ? 32 : (R < 2 ? 64 : 0))));
}
// rows per lane of the phase-1 kernel: 4 for n <= 4; 2 beyond (groups twice as wide), which keeps the extra column
// and the carried cost row within two waves per SIMD
constexpr int lp_p1_rows(int n) { return n <= 4 ? 4 : 2; }

constexpr int LDS_MAXC = 32;  // column slots of the LDS engine (n <= 17 structural + artificial)
// LDS bytes one LP of (m_max, columns nc) needs; 0 when it does not fit a workgroup (160 KB per CU on gfx950)
constexpr size_t lds_lp_bytes(int m_max, int nc) {
    const int ld = nc | 1;
    const size_t need = (size_t)m_max * ld * 8 + (size_t)m_max * 24 + 3 * LDS_MAXC * 8 + LDS_MAXC * 4 + 64;
    return need <= 160 * 1024 ? ((need + 15) & ~(size_t)15) : 0;
}
// resident wavefronts: limited by LDS per CU and 8 single-wave workgroups per SIMD-set; the loop strides the rest
constexpr int lds_grid(long long B, size_t smem) {
    long long per_cu = (long long)(160 * 1024 / smem);
    if (per_cu > 32) per_cu = 32;
    if (per_cu < 1) per_cu = 1;
    long long blocks = 256 * per_cu * 4;
    if (blocks > B) blocks = B;
    return (int)(blocks < 1 ? 1 : blocks);
}

// ------------------------------------------------------------------------------------------- the plans
enum LpEngine : int {
    LE_NONE = 0,   // unsupported size (the launchers return 2)
    LE_EMPTY,      // pairs only: nothing to launch, success
    LE_LDS,        // lp_lds_kernel / cheby_lds_kernel: one LP per wavefront, dictionary in `lds` bytes
    LE_WIDE,       // lp_w_kernel<N> / cheby_w_kernel<D> / adjacent_w_kernel<D>: one LP per wavefront;
                   // boxes: bbox_lazy_kernel<D, dense> (nw = 1) or bbox_wsplit_kernel<D, 4, dense> (nw = 4)
    LE_GROUP,      // lp_r_kernel<N, gs> / cheby_r_kernel<D, gs> / bbox_r_kernel<D, gs> / adjacent_r_kernel<D, gs>
    LE_GENERAL,    // lp_kernel<N> / cheby_kernel<D>: gs lanes per LP, one row per lane
    LE_LANE,       // boxes: bbox_lane_kernel<D, gs, rows> (rows: row slots per polytope, 16 / 32)
    LE_SPLIT,      // boxes: bbox_split_kernel<D, gs>, the latency form of the lane groups
};

// one launch, in the record of plp_reduce_plan.hpp: engine, gs (lanes per LP), rows (per lane; LE_LANE: row slots per polytope), nw and dense (boxes, LE_WIDE:
// wavefronts per polytope, 1 / 4, and whether the 2d LPs keep a stored dictionary), grid, block, lds (dynamic bytes)
using LpLaunch = ReduceLaunch;

struct LpPlan {
    LpLaunch first;       // LE_NONE: unsupported
    bool p1 = false;      // LE_GROUP: lp_p1_r_kernel<N, p1_launch.gs, p1_launch.rows> follows on the same stream
    LpLaunch p1_launch;
    bool second = false;  // ... and then the general kernel's retry pass (phase 1 reports `more`)
    LpLaunch retry;       // that pass: lp_kernel<N> with retry_only, its grid capped at 256 * 8
};
struct ChebyPlan {
    LpLaunch first;
    int force_retry = 0;  // PLP_CHEBY_RETRY_ALL=1 (LE_GROUP)
};
struct BoxPlan {
    LpLaunch first;
    int force_retry = 0;
    int handover = 0;     // what the launch can give the verifier: 0 nothing, 1 bases + centres, 2 final points (BoxHandover)
};
struct PairPlan {
    LpLaunch first;       // LE_EMPTY: n == 0 or an empty range
    int force_retry = 0;
    long long p_lo = 0, p_hi = 0;  // the pair range the kernel gets (the matrix form: every pair)
};

// The A/B switches: each the value of its variable, nullptr when unset.
struct LpEnv {
    const char* lds = nullptr;               // PLP_LDS
    const char* lp_wide = nullptr;           // PLP_LP_WIDE
    const char* lp_1row = nullptr;           // PLP_LP_1ROW
    const char* cheby_wide = nullptr;        // PLP_CHEBY_WIDE
    const char* cheby_1row = nullptr;        // PLP_CHEBY_1ROW
    const char* retry_all = nullptr;         // PLP_CHEBY_RETRY_ALL
    const char* bbox_lane = nullptr;         // PLP_BBOX_LANE
    const char* bbox_split = nullptr;        // PLP_BBOX_SPLIT
    const char* bbox_wide = nullptr;         // PLP_BBOX_WIDE
    const char* bbox_wsplit = nullptr;       // PLP_BBOX_WSPLIT
    const char* bbox_wsplit_maxb = nullptr;  // PLP_BBOX_WSPLIT_MAXB
    const char* bbox_wdense = nullptr;       // PLP_BBOX_WDENSE
    const char* adj_wide = nullptr;          // PLP_ADJ_WIDE
};

// read once per call (tests change the switches between the calls of one process)
inline LpEnv lp_env() {
    LpEnv e;
    e.lds = getenv("PLP_LDS");
    e.lp_wide = getenv("PLP_LP_WIDE");
    e.lp_1row = getenv("PLP_LP_1ROW");
    e.cheby_wide = getenv("PLP_CHEBY_WIDE");
    e.cheby_1row = getenv("PLP_CHEBY_1ROW");
    e.retry_all = getenv("PLP_CHEBY_RETRY_ALL");
    e.bbox_lane = getenv("PLP_BBOX_LANE");
    e.bbox_split = getenv("PLP_BBOX_SPLIT");
    e.bbox_wide = getenv("PLP_BBOX_WIDE");
    e.bbox_wsplit = getenv("PLP_BBOX_WSPLIT");
    e.bbox_wsplit_maxb = getenv("PLP_BBOX_WSPLIT_MAXB");
    e.bbox_wdense = getenv("PLP_BBOX_WDENSE");
    e.adj_wide = getenv("PLP_ADJ_WIDE");
    return e;
}
inline int lp_force_retry(const LpEnv& env) { return plan_detail::is(env.retry_all, '1') ? 1 : 0;  }

namespace plan_detail {

// the LDS engine (nc columns); LE_NONE when the dictionary does not fit
inline LpLaunch plan_lds(long long B, int m_max, int nc) {
    const size_t smem = m_max < 0 ? 0 : lds_lp_bytes(m_max < 1 ? 1 : m_max, nc);
    return smem ? launch(LE_LDS, 64, 1, lds_grid(B, smem), 64, smem) : LpLaunch();
}
// one LP per wavefront and workgroup: rows 1 .. 64, a grid of B; false: not this engine
inline bool plan_wave(long long B, int m_max, LpLaunch& L) {
    if (m_max < 1 || m_max > LP_MAX_M || B > LP_MAX_GRID) return false;
    L = launch(LE_WIDE, 64, 1, at_least1(B), 64, 0);
    return true;
}
// lane groups of R rows per lane, 64 / gs LPs per workgroup over `count` LPs and at least `min_grid` workgroups
inline bool plan_lane_group(long long count, int rows, int R, long long min_grid, LpLaunch& L) {
    const int gs = lp_group_size(R, rows);
    if (rows < 1 || !gs) return false;
    long long blocks = cdiv(count, RBLK / gs);
    if (blocks < min_grid) blocks = min_grid;
    if (blocks > LP_MAX_GRID) return false;
    L = launch(LE_GROUP, gs, R, at_least1(blocks), RBLK, 0);
    return true;
}
// one row per lane, one LP tile per block: the dispatcher balances uneven pivot counts
inline LpLaunch plan_general(long long B, int m_max) {
    const int gs = group_size_for(m_max);
    long long blocks = cdiv(B, LP_GENERAL_BLOCK / gs);
    if (blocks > (1ll << 20)) blocks = 1ll << 20;
    return launch(LE_GENERAL, gs, 1, at_least1(blocks), LP_GENERAL_BLOCK, 0);
}

// the engine of `count` pair LPs over n cells of up to m_max rows each (L stays LE_NONE when none applies):
// d >= 9 (no lane-group kernel), and d = 5..8 when the stacked pair has more than 32 rows or the pairs are few: one
// pair per wavefront (plp_wide.hip), the rule of the Chebyshev batches.  PLP_ADJ_WIDE=0 / 1: A/B, tests
inline void plan_pair_engine(long long count, int n, int m_max, int d, bool compact, const LpEnv& env, LpLaunch& L) {
    const bool wide = d > 8 || (d >= 5 && (env.adj_wide ? env.adj_wide[0] == '1'
                                                        : (2 * m_max > ADJ_WIDE_MIN_ROWS || count <= ADJ_WIDE_SMALL_PAIRS)));
    const long long wdiag = compact ? 0 : cdiv(n, 64);
    const long long wblocks = at_least1(count > wdiag ? count : wdiag);
    if (wide && wblocks <= LP_MAX_GRID) {
        L = launch(LE_WIDE, 64, 1, wblocks, 64, 0);
        return;
    }
    if (d <= 8) plan_lane_group(count, 2 * m_max, 4, compact ? 0 : cdiv(n, RBLK), L);
}

}  // namespace plan_detail

// ---- generic LPs  min c'x  s.t.  G x <= h  (plp_lp_solve_batch)
inline LpPlan plan_lp(long long B, int m_max, int n, const LpEnv& env) {
    using namespace plan_detail;
    LpPlan p;
    if (n < 1 || n > LP_MAX_D + 1 || m_max < 0) return p;
    // more than 64 rows (or PLP_LDS=1: A/B, tests): the LDS-resident engine, one LP per wavefront (plp_lds.hip)
    if (m_max > LP_MAX_M || is(env.lds, '1')) {
        p.first = plan_lds(B, m_max, n + 1);
        return p;
    }
    // n = 5..16: both phases in one kernel, nothing is handed over.  PLP_LP_WIDE=0 / 1: never / always (A/B, tests)
    const bool wide = env.lp_wide ? env.lp_wide[0] == '1' : !is(env.lp_1row, '1');
    if (n >= 5 && n <= LP_MAX_D && wide && plan_wave(B, m_max, p.first)) return p;
    // the second pass mostly reads statuses: a grid-stride sweep
    p.retry = plan_general(B, m_max);
    if (p.retry.grid > 256 * 8) p.retry.grid = 256 * 8;
    // LPs whose origin is feasible (no phase 1) are solved by the lane groups; they mark the others ST_RETRY, the phase-1
    // kernel takes those it can (n = 3..4) and the general kernel's second pass redoes exactly what is left
    // (PLP_LP_1ROW=1 keeps everything on the general kernel: A/B, tests)
    if (!is(env.lp_1row, '1') && B >= 1 && plan_lane_group(B, m_max, lp_rows_per_lane(n), 0, p.first)) {
        p.second = true;
        if (n >= 3 && n <= PLP_P1_FAST_MAXN) {
            p.p1 = true;
            const int rp = lp_p1_rows(n), gsp = p.first.gs * p.first.rows / rp;  // same row slots, rp rows per lane
            p.p1_launch = launch(LE_GROUP, gsp, rp, at_least1(cdiv(B, RBLK / gsp)), RBLK, 0);
        }
        return p;
    }
    p.first = plan_general(B, m_max);
    return p;
}

// ---- Chebyshev balls (plp_cheby_batch)
inline ChebyPlan plan_cheby(long long B, int m_max, int d, const LpEnv& env) {
    using namespace plan_detail;
    ChebyPlan p;
    p.force_retry = lp_force_retry(env);
    if (d < 1 || d > LP_MAX_D || m_max < 0) return p;
    if (m_max > LP_MAX_M || is(env.lds, '1')) {
        p.first = plan_lds(B, m_max, d + 1);
        return p;
    }
    // large shapes: one LP per wavefront with a wave-uniform pivot column (plp_wide.hip); PLP_CHEBY_WIDE=0 keeps the
    // lane-group kernels, PLP_CHEBY_WIDE=1 sends every shape it supports (d >= 5) there: A/B, tests
    const bool wide = env.cheby_wide ? env.cheby_wide[0] == '1'
                                     : (d >= PLP_WIDE_MIN_D && (m_max > PLP_WIDE_MIN_M || B <= PLP_WIDE_SMALL_B));
    if (wide && d >= 5 && plan_wave(B, m_max, p.first)) return p;
    // four rows per lane, two from d = 9 (PLP_CHEBY_1ROW=1 keeps the one-row-per-lane kernel: A/B, tests)
    if (!is(env.cheby_1row, '1') && plan_lane_group(B, m_max, lp_rows_per_lane(d), 0, p.first)) return p;
    p.first = plan_general(B, m_max);
    return p;
}

// ---- bounding boxes: the Chebyshev LP + 2d LPs from its centre per polytope (plp_bbox_batch)
inline BoxPlan plan_bbox(long long B, int m_max, int d, const LpEnv& env) {
    using namespace plan_detail;
    BoxPlan p;
    p.force_retry = lp_force_retry(env);
    if (m_max < 1 || m_max > LP_MAX_M || B < 1 || d < 1 || d > LP_MAX_D) return p;
    p.handover = 1;
    // up to 32 rows in d <= 3: the 2d box LPs one LP per lane (plp_bbox_lane.hip), with the tile shapes of the fused
    // reduce; PLP_BBOX_LANE=0: never (A/B); PLP_BBOX_SPLIT set: the lane-group forms keep their A/B meaning
    if (d <= BBOX_LANE_MAXD && m_max <= BBOX_LANE_MAXM && !is(env.bbox_lane, '0') && !env.bbox_split && B <= LP_MAX_GRID) {
        const int rows = m_max > 16 ? 32 : 16;
        const int gs = rows == 32 ? (B <= PLP_REDUCE_LANE32_GS16_MAXB ? 16 : 8)
                                  : (B <= PLP_REDUCE_LANE_GS16_MAXB ? 16 : (B <= PLP_REDUCE_LANE_GS8_MAXB ? 8 : 4));
        p.first = launch(LE_LANE, gs, rows, cdiv(B, 64 / gs), RBLOCK, reduce_lane_smem_bytes(d, gs, rows));
        p.handover = 2;
        return p;
    }
    // one polytope per wavefront: d = 9..16 always; d = 5..8 by the thresholds above (PLP_BBOX_WIDE=0 / 1: never / always)
    const bool small_batch = !env.bbox_wide && !env.bbox_split && !env.bbox_wsplit && B <= BBOX_WIDE_SMALL_B;
    const bool wide = d > 8 || (d >= 5 && (env.bbox_wide ? env.bbox_wide[0] == '1'
                                                         : ((m_max > BBOX_WIDE_MIN_M && B > BBOX_WIDE_MIN_B) || small_batch)));
    if (wide && B <= LP_MAX_GRID) {
        // small batches: four wavefronts per polytope (PLP_BBOX_WSPLIT=0 / 1: never / always; PLP_BBOX_WSPLIT_MAXB)
        const long long maxb = env.bbox_wsplit_maxb ? atoll(env.bbox_wsplit_maxb) : PLP_BBOX_WSPLIT_MAXB;
        const bool four = is(env.bbox_wsplit, '1') || (!is(env.bbox_wsplit, '0') && B <= maxb);
        p.first = launch(LE_WIDE, 64, 1, B, four ? 256 : 64, 0);
        p.first.nw = four ? 4 : 1;
        // PLP_BBOX_WDENSE=0 / 1: never / always the dense engine for the 2d LPs (A/B)
        p.first.dense = env.bbox_wdense ? env.bbox_wdense[0] == '1' : (d <= PLP_BBOX_WDENSE_MAXD);
        return p;
    }
    // lane groups, four rows per lane (d <= 8).  Small batches: one polytope per wavefront, its 2d LPs over the lane groups
    // (PLP_BBOX_SPLIT=0 / 1: never / always)
    if (d <= 8) {
        const int gs = lp_group_size(4, m_max);
        if (is(env.bbox_split, '1') || (!is(env.bbox_split, '0') && B <= bbox_split_maxb(gs))) {
            p.first = launch(LE_SPLIT, gs, 4, B, RBLK, 0);
            return p;
        }
        if (plan_lane_group(B, m_max, 4, 0, p.first)) return p;
    }
    p.handover = 0;
    return p;
}

// ---- pair LPs: the two cells of a pair stacked (plp_adjacent_pairs, _range, plp_overlap_pairs, plp_overlap_cross)
// compact: pairs [p_lo, p_hi) into a list; else all pairs into the n x n matrix, whose diagonal the first
// ceil(n / 64) workgroups write; cross_n1 > 0 (compact only): pairs of the first cross_n1 cells with the others
inline PairPlan plan_pairs(int n, int m_max, int d, long long p_lo, long long p_hi, bool compact, int cross_n1,
                           const LpEnv& env) {
    using namespace plan_detail;
    PairPlan p;
    p.force_retry = lp_force_retry(env);
    if (n < 0 || m_max < 1 || 2 * m_max > LP_MAX_M || d < 1 || d > LP_MAX_D) return p;
    if (cross_n1 < 0 || cross_n1 > n || (cross_n1 > 0 && !compact)) return p;
    const long long npairs = cross_n1 > 0 ? (long long)cross_n1 * (n - cross_n1) : (long long)n * (n - 1) / 2;
    if (!compact) { p_lo = 0; p_hi = npairs; }
    if (p_lo < 0 || p_hi > npairs || p_lo > p_hi) return p;
    p.p_lo = p_lo;
    p.p_hi = p_hi;
    if (n == 0 || (compact && p_lo == p_hi)) {
        p.first.engine = LE_EMPTY;
        return p;
    }
    plan_pair_engine(p_hi - p_lo, n, m_max, d, compact, env, p.first);
    return p;
}

// ---- the listed form (plp_pair_list): K pairs of the n cells, each named by its two indices; the engines and the rule that
// picks among them are plan_pairs', sized by K (a list may name a pair more than once: K has no bound but the grid's)
inline PairPlan plan_pair_list(int n, int m_max, int d, long long K, const LpEnv& env) {
    using namespace plan_detail;
    PairPlan p;
    p.force_retry = lp_force_retry(env);
    if (n < 0 || m_max < 1 || 2 * m_max > LP_MAX_M || d < 1 || d > LP_MAX_D || K < 0) return p;
    p.p_hi = K;
    if (K == 0) {
        p.first.engine = LE_EMPTY;
        return p;
    }
    plan_pair_engine(K, n, m_max, d, true, env, p.first);
    return p;
}

}  // namespace plp
