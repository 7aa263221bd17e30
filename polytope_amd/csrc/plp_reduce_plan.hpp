// plp_reduce_plan.hpp -- which kernel the fused reduce() runs for a batch, decided in one place.
//
// plan_reduce(B, m_max, d, env) is a pure host function (no HIP): it names the engine of the first launch, its tile shape,
// grid, workgroup and LDS bytes, and whether the second pass of the general kernel (reduce_kernel, plp_reduce_general.hpp:
// one row per lane, Bland's rule) has to redo what the first launch hands back (RF_RETRY).  The launchers
// (plp_reduce_launch.hpp) only carry the plan out.  tests/test_reduce_plan.py pins it on the CPU.
//
// The engines, by shape (defaults):
//   d <= 4, m <= 32     one LP per lane (reduce_lane_kernel / reduce_lane_mix_kernel, plp_reduce_lane.hpp), complete;
//                       d = 4 only beyond PLP_REDUCE_LANE4_MINB*, below that the lane-group forms of d <= 8
//   d <= 8              four rows per lane, groups of 4 / 8 / 16 lanes (reduce_r_kernel, plp_reduce_r_impl.hpp); small
//                       batches one polytope per wavefront (reduce_split_kernel); m <= 16, d <= 4: reduce_r_mix_kernel
//   d = 5..8            beyond the latency form's batch sizes two rows per lane; more than 32 rows, or up to
//                       PLP_REDUCE_WG_MAXB polytopes: one polytope per wavefront / workgroup (wdense, wsplit)
//   d = 9..16           two rows per lane, groups of 16 / 32 lanes; more than 32 rows, or up to PLP_REDUCE_WG_MAXB
//                       polytopes: one polytope per wavefront (wdense up to PLP_REDUCE_WDENSE_MAXD, lazy beyond) or
//                       per workgroup (wsplit)
// A/B switches (environment, read once per call by reduce_env()):
//   PLP_REDUCE_1ROW=1        the general kernel alone
//   PLP_REDUCE_LANE=0/1      d <= 4, m <= 32: never / always one LP per lane
//   PLP_REDUCE_LANE_GS=4/8/16, PLP_REDUCE_LANE_MIX=k   that tile shape whatever the batch size / k/64 of the tiles short
//   PLP_REDUCE_SPLIT=0/1     never / always the latency form (set at all: no lane engine, no small-batch one-per-workgroup form)
//   PLP_REDUCE_HALF=0/1      m <= 16, d <= 4 lane-group form: never / always half-size tiles up to 4096 tiles (set at all:
//                            no lane engine, no small-batch form)
//   PLP_REDUCE_LAZY=0/1      d >= 5: never / always one polytope per wavefront
//   PLP_REDUCE_WDENSE=0/1    ... its LPs without / with a stored dictionary
//   PLP_REDUCE_WSPLIT=0/2/4  ... never / always 2 / 4 wavefronts per polytope
//   PLP_REDUCE_R1=1          d > 8, m > 32: one row per lane, 64 lanes per polytope (set at all: no small-batch form)
//   PLP_REDUCE_R2=0          d > 8: the general kernel alone
//   PLP_REDUCE_RETRY_ALL=1   every polytope through the second pass (the fast kernels hand all of them back)
#pragma once
#include <stddef.h>
#include <stdlib.h>

namespace plp {

#ifndef PLP_REDUCE_R_BLOCK
// One wavefront per workgroup: at C2 (100000 polytopes = 6250 wavefronts over 4096 resident slots) the last
// round is spread over the CUs wave by wave instead of in blocks of four (measured 256: 0.306 ms, 128: 0.305,
// 64: 0.299), and the workgroup barriers cost nothing.
#define PLP_REDUCE_R_BLOCK 64
#endif
constexpr int RBLOCK = PLP_REDUCE_R_BLOCK;  // threads per workgroup of every kernel below but the general one
constexpr int REDUCE_GENERAL_BLOCK = 256;   // threads per workgroup of reduce_kernel (= BLOCK, plp_common.hpp)

// ------------------------------------------------------------------------------------------- thresholds
// d >= 5, any row count: one polytope per workgroup (wsplit) / wavefront up to this many polytopes.  Round 4: one polytope
// per workgroup, its LPs on 2 / 4 wavefronts (reduce_wsplit_kernel), is 1.15x .. 2x ahead of the lane-group kernels up to
// ~1 000 polytopes at every (m <= 32, d) measured, level at 2 000 .. 4 000, behind beyond (scripts/debug/mid_wsplit_table.py)
#ifndef PLP_REDUCE_WG_MAXB
#define PLP_REDUCE_WG_MAXB 1500
#endif

// (16,3)-class batches larger than this: one LP per lane; its 4-polytope tiles are ahead of the lane-group latency form
// down to a single polytope
#ifndef PLP_REDUCE_LANE_MINB
#define PLP_REDUCE_LANE_MINB 0
#endif
// d = 4 (the walk in R^4, three waves per SIMD) -- measured after the walk's direction with three active rows became a
// generalised cross product (scripts/debug/lane_d4_sweep.py, us lane-group / lane): (8,4) x 20 000 21 / 24, x 50 000 51 / 37;
// (12,4) x 10 000 37 / 39, x 30 000 63 / 68, x 50 000 99 / 76; (16,4) x 2 000 43 / 44, x 5 000 68 / 51, x 10 000 87 / 70,
// x 50 000 209 / 150; (20,4) x 2 000 61 / 58, x 5 000 102 / 75, x 50 000 359 / 276; (32,4) x 500 57 / 60, x 2 000 79 / 63,
// x 5 000 144 / 89, x 10 000 183 / 123, x 50 000 483 / 325
#ifndef PLP_REDUCE_LANE4_MINB
#define PLP_REDUCE_LANE4_MINB 40000   // d = 4, fewer than 14 rows: batches larger than this
#endif
#ifndef PLP_REDUCE_LANE4_MINB_ROWS14
#define PLP_REDUCE_LANE4_MINB_ROWS14 3000   // d = 4, 14..32 rows: batches larger than this
#endif

// Lane engine, tile shape by batch size, measured on (16,3) batches (scripts/debug/lane_sweep.py, us per launch GS 4 / 8 / 16):
//   B = 3 000: 51 / 35 / 27.5    8 000: 56 / 38 / 34    12 000: 58 / 46 / 41    16 000: 58 / 47 / 49    20 000: 66 / 56 / 62
//   30 000: 71 / 69 / 81    40 000: 89 / 88 / 101    (lane-group kernels: 40 / 48 / 60 / 62 / 75 / 91 / 106)
#ifndef PLP_REDUCE_LANE32_GS16_MAXB
#define PLP_REDUCE_LANE32_GS16_MAXB 16000  // 17..32 rows: batches up to this size on 4 polytopes per wavefront
#endif
#ifndef PLP_REDUCE_LANE_GS8_MAXB
#define PLP_REDUCE_LANE_GS8_MAXB 40000   // batches up to this size: 8 polytopes per wavefront
#endif
#ifndef PLP_REDUCE_LANE_GS16_MAXB
#define PLP_REDUCE_LANE_GS16_MAXB 14000  // ... up to this size: 4 polytopes per wavefront
#endif
// Larger batches: 16 polytopes per wavefront, the LAST eighth of the tiles (at most 1024) as 8-polytope tiles.  The
// workgroups of a launch are handed out over tens of microseconds and the launch ends when the ones that started last
// end: short tiles there cut 12 us off 50 000 .. 100 000 polytopes (100 000: 166 us without, 153-155 with 2/64 .. 8/64 of
// the tiles, 159-172 beyond 12/64; 50 000: 104 -> 91).  PLP_REDUCE_LANE_MIX=k: k / 64 of the tiles (0: none).
// (d = 4: the short tiles do not pay at 32 row slots, (20,4) x 50 000: 315 us with, 300 without)
#define PLP_REDUCE_LANE_MIX_DIV 8        // the last 1/8 of the tiles ...
#define PLP_REDUCE_LANE_MIX_MAXTAIL 1024 // ... at most this many
#define PLP_REDUCE_LANE_MIX_MINBLOCKS 512

// Lane-group latency form (reduce_split_kernel): batches up to this size.  Measured (device time per call, batch form ->
// latency form): (16,3) B = 1: 49 -> 21 us, 256: 77 -> 25, 4096: 81 -> 50, 16384: 90 -> 153; (32,6) 256: 274 -> 79,
// 4096: 306 -> 202; (64,8) 256: 652 -> 257, 4096: 896 -> 728; (16,8) 256: 80 -> 75, 4096: 82 -> 111 (16 rows at d >= 7 gain
// nothing: the 2d box LPs already fill the 16 groups).  ~20 us of every figure are the launches of a call.
// (round 3, with the F2 presolve and d = 5..8 on two rows per lane beyond this size: (32,6) B = 2048: 0.121 ms here vs 0.181,
// B = 4096: 0.222 vs 0.187; (64,8) B = 1024: 0.302 vs 0.366, B = 2000: 0.426 vs 0.404)
#ifndef PLP_REDUCE_SPLIT_MAXB
#define PLP_REDUCE_SPLIT_MAXB(D, GS) \
    ((((GS) == 4 && (D) >= 7) || (D) > 8 || ((D) >= 5 && (GS) == 16)) ? 1024 : ((D) >= 5 ? 2048 : 4096))  // (d > 8: four groups only; (32,12) B = 4096: 154 -> 201 us)
#endif

// reduce_r_mix_kernel (m <= 16, d <= 4 on lane groups): more tiles than the chip holds at once (4096 wavefront slots): the
// last 1/32 of the tiles (at most 1024) are split into half-size ones.  Measured at C2 (6250 tiles): 0.2765 ms without,
// 0.2579-0.2609 ms with 2/64 .. 9/64 of the batch in half-size tiles (a flat optimum), 0.27-0.29 ms beyond 10/64; round 4:
// 1/32 instead of 1/16 -- the optimum is flat between 2/64 and 8/64: 0.1908 / 0.1919 ms.  A third class of quarter-size
// tiles (16 lanes x 1 row) behind the half-size ones was measured too: no gain (0.2557-0.2602 ms for the last 2/256 ..
// 12/256 of the batch), not kept.  Medium batches (fewer full tiles than half the chip's wavefront slots): half-size tiles
// only -- twice the wavefronts, each done in about half the time.
#define PLP_REDUCE_MIX_DIV 32
#define PLP_REDUCE_MIX_MAXTAIL 1024
#define PLP_REDUCE_MIX_MINBLOCKS 4096   // more tiles than this: the tail of half-size tiles
#define PLP_REDUCE_HALF_MAXBLOCKS 2048  // up to this many tiles: half-size tiles only (PLP_REDUCE_HALF=1: up to 4096)

// One polytope per wavefront: F3 / F2 on the dense one-LP-per-wavefront engine up to this d, without a stored dictionary
// beyond (measured, scripts/debug/wdense_ab.py, 64 rows, B = 20 000, ms dense / lazy: d = 8 1.39 / 2.30, 12 1.66 / 1.90,
// 13 1.58 / 1.65, 14 1.48 / 1.48, 15 1.48 / 1.38, 16 1.60 / 1.33)
#ifndef PLP_REDUCE_WDENSE_MAXD
#define PLP_REDUCE_WDENSE_MAXD 13
#endif

// One polytope per workgroup of NW wavefronts (reduce_wsplit_kernel).  Measured (scripts/debug/wsplit_sweep.py, ms with
// one / two / four wavefronts per polytope):
//   (64,8)   B = 1  0.192 / 0.116 / 0.085    250  0.230 / 0.142 / 0.100    1 000  0.251 / 0.162 / 0.131    2 000  0.292 / 0.212 / 0.222
//            5 000  0.444 / 0.417 / 0.432    8 000  0.658 / 0.597 / 0.640    16 000  1.127 / 1.077 / 1.218
//   (48,6)   250  0.159 / 0.096 / 0.070    5 000  0.301 / 0.253 / 0.254    16 000  0.678 / 0.620 / 0.681
//   (64,12)  250  0.267 / 0.161 / 0.120    5 000  0.580 / 0.495 / 0.543    16 000  1.336 / 1.319 / 1.591
// With the presolve over the wavefronts: four ahead of two up to 12 000 polytopes at d <= 8 -- (64,8) 5 000 0.379 / 0.402,
// 12 000 0.803 / 0.810, 16 000 1.051 / 1.026 -- and up to ~3 000 at d = 9..13: (64,12) 3 000 0.338 / 0.366, 5 000 0.502 / 0.495.
// Without a stored dictionary, d = 14..16: (64,16) B = 250 0.228 / 0.143 / 0.112 ms, 1 000 0.248 / 0.170 / 0.201,
// 3 000 0.355 / 0.346 / 0.437, 8 000 0.704 / 0.703 / 0.951.
#define PLP_REDUCE_WS2_MAXB_DENSE 16000   // two wavefronts per polytope up to here (dense LPs)
#define PLP_REDUCE_WS4_MAXB_DENSE8 12000 // four up to here, d <= 8
#define PLP_REDUCE_WS4_MAXB_DENSE 2000   // four up to here, d = 9..13
#define PLP_REDUCE_WS2_MAXB_LAZY 3000     // two up to here (LPs without a stored dictionary)
#define PLP_REDUCE_WS4_MAXB_LAZY 500     // four up to here

// ------------------------------------------------------------------------------------------- tile shapes and LDS
// lanes per polytope of the general kernel (= group_size_for, plp_kernels.hpp)
constexpr int reduce_general_gs(int m_max) { return m_max <= 8 ? 8 : (m_max <= 16 ? 16 : (m_max <= 32 ? 32 : 64)); }
constexpr size_t reduce_smem_bytes(int gs, int D) {
    return ((size_t)(REDUCE_GENERAL_BLOCK / gs) * gs * (D + 1) * 8 + 15) & ~(size_t)15;
}
// lanes per polytope of the four-rows-per-lane kernel
constexpr int group_size_r(int m_max) { return m_max <= 16 ? 4 : (m_max <= 32 ? 8 : 16); }
// (bench shape on lane groups: 16 polytopes x 16 rows x 5 doubles = 10 240 B per one-wavefront workgroup, and 16 of them --
// four waves per SIMD -- are EXACTLY the CU's 160 KB: 384 B more per workgroup (the centres kept in LDS, tried in round 4
// against the spills) and a CU holds 15, 0.194 -> 0.213 ms)
constexpr size_t reduce_r_smem_bytes(int gs, int D, int R) {
    return ((size_t)(RBLOCK / gs) * gs * R * (D + 2) * 8 + 15) & ~(size_t)15;  // A rows, b, 1/||a||
}
constexpr size_t reduce_split_smem_bytes(int gs, int D, int R) {
    return (((size_t)gs * R * (D + 2) + 2 * D + 2) * 8 + 15) & ~(size_t)15;
}
// lane engine: ROWS row slots for each of the 64 / GS polytopes of a tile
constexpr size_t reduce_lane_smem_bytes(int D, int GS, int ROWS) { return (size_t)(64 / GS) * ROWS * (D + 2) * 8; }
// sizeof(wide::WideShared<D + 1>) (plp_wide.hpp; checked where the kernels are launched)
constexpr size_t wide_shared_bytes(int D) { return ((size_t)20 * (D + 2) + 7) & ~(size_t)7; }
constexpr size_t reduce_lazy_smem_bytes(int D) {   // reduce_lazy_kernel / reduce_wdense_kernel: rows + lazy::lds_bytes<D>
    return reduce_r_smem_bytes(64, D, 1) + ((wide_shared_bytes(D) + 255) & ~(size_t)255);
}
constexpr size_t reduce_wsplit_smem_bytes(int D, int NW) {   // + the presolve's masks and blocking rows
    return (size_t)64 * (D + 2) * 8 + (size_t)(D + 2 + 2 * D) * 8 + 8 * 8 + 8 * 4 + 64 * 4 +
           NW * ((wide_shared_bytes(D) + 15) & ~(size_t)15) + (size_t)2 * NW * 8 + (size_t)NW * 64 * 4;
}

// ------------------------------------------------------------------------------------------- the plan
enum ReduceEngine : int {
    RE_NONE = 0,    // (B, m_max, d) unsupported
    RE_GENERAL,     // reduce_kernel<D>, gs lanes per polytope: complete by itself
    RE_LANE,        // reduce_lane_kernel<D, gs, rows>   (rows: row slots per polytope, 16 / 32)
    RE_LANE_MIX,    // reduce_lane_mix_kernel<D, rows, gs, 2 gs>: nbig tiles of 64 / gs polytopes, then tiles of 32 / gs
    RE_GROUP,       // reduce_r_kernel<D, gs, rows>      (rows per lane: 4 / 2 / 1)
    RE_GROUP_MIX,   // reduce_r_mix_kernel<D>: nbig tiles of 4 lanes x 4 rows, then tiles of 8 lanes x 2 rows
    RE_SPLIT,       // reduce_split_kernel<D, gs, rows>: one polytope per wavefront
    RE_WDENSE,      // reduce_wdense_kernel<D>: one polytope per wavefront, dense LPs
    RE_LAZY,        // reduce_lazy_kernel<D>: one polytope per wavefront, LPs without a stored dictionary
    RE_WSPLIT,      // reduce_wsplit_kernel<D, nw, dense>: one polytope per workgroup of nw wavefronts
};

struct ReduceLaunch {
    int engine = RE_NONE;
    int gs = 0;          // lanes per polytope (lane-mix / group-mix: of the first nbig tiles)
    int rows = 0;        // rows per lane (RE_GROUP, RE_SPLIT), row slots per polytope (RE_LANE, RE_LANE_MIX)
    int nw = 0;          // RE_WSPLIT: wavefronts per polytope
    int dense = 0;       // RE_WSPLIT: the dense LP engine
    long long nbig = 0;  // RE_LANE_MIX, RE_GROUP_MIX: workgroups with the full-size tiles
    long long grid = 0;  // workgroups
    int block = 0;       // threads per workgroup
    size_t lds = 0;      // dynamic LDS bytes
};

struct ReducePlan {
    ReduceLaunch first;    // engine RE_NONE: unsupported
    bool second = false;   // the general kernel's second pass follows `first` (false: `first` is complete)
    ReduceLaunch retry;    // that pass: reduce_kernel<D> over the polytopes flagged RF_RETRY
    int force_retry = 0;   // PLP_REDUCE_RETRY_ALL=1: the fast kernels hand every polytope back
};

// The A/B switches: each the value of its variable, nullptr when unset.  A switch "is set" whatever its value.
struct ReduceEnv {
    const char* lane = nullptr;       // PLP_REDUCE_LANE
    const char* lane_gs = nullptr;    // PLP_REDUCE_LANE_GS
    const char* lane_mix = nullptr;   // PLP_REDUCE_LANE_MIX
    const char* retry_all = nullptr;  // PLP_REDUCE_RETRY_ALL
    const char* one_row = nullptr;    // PLP_REDUCE_1ROW
    const char* r1 = nullptr;         // PLP_REDUCE_R1
    const char* r2 = nullptr;         // PLP_REDUCE_R2
    const char* lazy = nullptr;       // PLP_REDUCE_LAZY
    const char* split = nullptr;      // PLP_REDUCE_SPLIT
    const char* half = nullptr;       // PLP_REDUCE_HALF
    const char* wsplit = nullptr;     // PLP_REDUCE_WSPLIT
    const char* wdense = nullptr;     // PLP_REDUCE_WDENSE
};

// read once per call (tests change the switches between the calls of one process)
inline ReduceEnv reduce_env() {
    ReduceEnv e;
    e.lane = getenv("PLP_REDUCE_LANE");
    e.lane_gs = getenv("PLP_REDUCE_LANE_GS");
    e.lane_mix = getenv("PLP_REDUCE_LANE_MIX");
    e.retry_all = getenv("PLP_REDUCE_RETRY_ALL");
    e.one_row = getenv("PLP_REDUCE_1ROW");
    e.r1 = getenv("PLP_REDUCE_R1");
    e.r2 = getenv("PLP_REDUCE_R2");
    e.lazy = getenv("PLP_REDUCE_LAZY");
    e.split = getenv("PLP_REDUCE_SPLIT");
    e.half = getenv("PLP_REDUCE_HALF");
    e.wsplit = getenv("PLP_REDUCE_WSPLIT");
    e.wdense = getenv("PLP_REDUCE_WDENSE");
    return e;
}

namespace plan_detail {

inline bool is(const char* s, char c) { return s && s[0] == c; }
inline long long cdiv(long long a, long long b) { return (a + b - 1) / b; }
inline long long at_least1(long long v) { return v < 1 ? 1 : v; }

inline ReduceLaunch launch(int engine, int gs, int rows, long long grid, int block, size_t lds) {
    ReduceLaunch L;
    L.engine = engine;
    L.gs = gs;
    L.rows = rows;
    L.grid = grid;
    L.block = block;
    L.lds = lds;
    return L;
}

// d <= 4, m <= 32: one LP per lane; complete
inline bool plan_lane(long long B, int m_max, int d, const ReduceEnv& env, ReduceLaunch& L) {
    if (B > 2147483647ll) return false;
    const char* eg = env.lane_gs;   // a forced shape is that shape only
    const int rows = m_max > 16 ? 32 : 16;
    int gs;
    if (rows == 32) gs = eg ? (atoi(eg) == 16 ? 16 : 8) : (B <= PLP_REDUCE_LANE32_GS16_MAXB ? 16 : 8);
    else if (eg) gs = atoi(eg) == 16 ? 16 : (atoi(eg) == 8 ? 8 : 4);
    else gs = B <= PLP_REDUCE_LANE_GS16_MAXB ? 16 : (B <= PLP_REDUCE_LANE_GS8_MAXB ? 8 : 4);
    const long long ng = 64 / gs;
    const long long blocks = at_least1(cdiv(B, ng));
    L = launch(RE_LANE, gs, rows, blocks, RBLOCK, reduce_lane_smem_bytes(d, gs, rows));
    if (gs != (rows == 32 ? 8 : 4)) return true;   // short tiles behind the throughput shape only
    long long tail = blocks / PLP_REDUCE_LANE_MIX_DIV < PLP_REDUCE_LANE_MIX_MAXTAIL ? blocks / PLP_REDUCE_LANE_MIX_DIV
                                                                                    : PLP_REDUCE_LANE_MIX_MAXTAIL;
    if (env.lane_mix) tail = blocks * atoi(env.lane_mix) / 64;
    if (eg || (rows == 32 && d == 4)) tail = 0;
    if (tail > 0 && blocks > PLP_REDUCE_LANE_MIX_MINBLOCKS) {
        L.engine = RE_LANE_MIX;
        L.nbig = blocks - tail;
        L.grid = L.nbig + cdiv(B - L.nbig * ng, ng / 2);
    }
    return true;
}

// one polytope per wavefront (wdense / lazy) or per workgroup of 2 / 4 wavefronts (wsplit)
inline bool plan_lazy(long long B, int d, const ReduceEnv& env, ReduceLaunch& L, bool& complete) {
    if (B > 2147483647ll) return false;
    const bool dense = env.wdense ? env.wdense[0] == '1' : (d <= PLP_REDUCE_WDENSE_MAXD);
    // complete: the dense LPs carry Bland's rule inside, no polytope is handed to a second pass (at small batches the idle
    // second launch was 5 % of the call)
    complete = dense && !is(env.retry_all, '1');
    const long long maxb = dense ? PLP_REDUCE_WS2_MAXB_DENSE : PLP_REDUCE_WS2_MAXB_LAZY;
    const long long maxb4 = dense ? (d <= 8 ? PLP_REDUCE_WS4_MAXB_DENSE8 : PLP_REDUCE_WS4_MAXB_DENSE)
                                  : PLP_REDUCE_WS4_MAXB_LAZY;
    const char* ws = env.wsplit;
    int nw = 0;
    if (B >= 1 && !is(ws, '0')) {
        if (is(ws, '4') || (!ws && B <= maxb4)) nw = 4;
        else if (is(ws, '2') || (!ws && B <= maxb)) nw = 2;
    }
    // (the wsplit kernel exists with the dense engine up to PLP_REDUCE_WDENSE_MAXD and without it beyond)
    if (nw && dense == (d <= PLP_REDUCE_WDENSE_MAXD)) {
        L = launch(RE_WSPLIT, 64, 1, B, 64 * nw, reduce_wsplit_smem_bytes(d, nw));
        L.nw = nw;
        L.dense = dense;
        return true;
    }
    L = launch(dense ? RE_WDENSE : RE_LAZY, 64, 1, at_least1(B), RBLOCK, reduce_lazy_smem_bytes(d));
    return true;
}

// lane groups of GS lanes, R rows per lane
inline bool plan_group(long long B, int d, int GS, int R, const ReduceEnv& env, ReduceLaunch& L) {
    const long long NG = RBLOCK / GS;
    long long blocks = cdiv(B, NG);
    if (blocks > 2147483647ll) return false;   // grid.x limit (never reached for realistic batches)
    blocks = at_least1(blocks);
    const size_t smem = reduce_r_smem_bytes(GS, d, R);
    if ((R == 4 && d <= 8) || (R == 2 && d > 8)) {
        // small batches: one polytope per wavefront, LPs in parallel
        if (is(env.split, '1') || (!is(env.split, '0') && B <= PLP_REDUCE_SPLIT_MAXB(d, GS))) {
            L = launch(RE_SPLIT, GS, R, at_least1(B), RBLOCK, reduce_split_smem_bytes(GS, d, R));
            return true;
        }
    }
    if (GS == 4 && R == 4 && d <= 4) {
        const size_t smem2 = reduce_r_smem_bytes(8, d, 2);
        const size_t smix = smem > smem2 ? smem : smem2;
        if (blocks <= 2 * PLP_REDUCE_HALF_MAXBLOCKS &&
            (is(env.half, '1') || (!is(env.half, '0') && blocks <= PLP_REDUCE_HALF_MAXBLOCKS))) {
            L = launch(RE_GROUP_MIX, GS, R, cdiv(B, NG / 2), RBLOCK, smix);
            return true;
        }
        if (blocks > PLP_REDUCE_MIX_MINBLOCKS) {
            const long long tail = blocks / PLP_REDUCE_MIX_DIV < PLP_REDUCE_MIX_MAXTAIL ? blocks / PLP_REDUCE_MIX_DIV
                                                                                      : PLP_REDUCE_MIX_MAXTAIL;
            L = launch(RE_GROUP_MIX, GS, R, 0, RBLOCK, smix);
            L.nbig = blocks - tail;
            L.grid = L.nbig + cdiv(B - L.nbig * NG, NG / 2);
            return true;
        }
    }
    L = launch(RE_GROUP, GS, R, blocks, RBLOCK, smem);
    return true;
}

// the first launch on a fast engine; false: none applies, the general kernel takes the batch
inline bool plan_fast(long long B, int m_max, int d, const ReduceEnv& env, ReduceLaunch& L, bool& complete) {
    complete = false;
    if (m_max < 1 || m_max > 64 || d < 1 || d > 16) return false;
    if (d <= 4 && m_max <= 32) {
        // up to 32 rows in d <= 4 (the bench shape; the stacks of Polytope.intersect): F3 / F2 one LP per lane
        const long long minb = d == 4 ? (m_max >= 14 ? PLP_REDUCE_LANE4_MINB_ROWS14 : PLP_REDUCE_LANE4_MINB) : PLP_REDUCE_LANE_MINB;
        const bool other = env.split || env.half;   // a switch of the lane-group forms keeps them
        if (is(env.lane, '1') || (!is(env.lane, '0') && !other && B > minb)) {
            complete = true;   // what the fast path hands back is redone inside the kernel
            return plan_lane(B, m_max, d, env, L);
        }
    }
    if (d > 8) {
        if (is(env.r2, '0')) return false;
        if (is(env.r1, '1') && m_max > 32) return plan_group(B, d, 64, 1, env, L);
        // more than 32 rows: one polytope per wavefront -- measured 1.2x (48 rows, d = 9) to 2.1x (36 rows, d = 14) faster
        // than two rows per lane, outputs bitwise equal; with 32 rows and fewer the four-polytopes-per-wavefront form wins or ties
        const bool small_batch = !env.lazy && B <= PLP_REDUCE_WG_MAXB && !(env.r1 && env.r1[0]);
        if (is(env.lazy, '1') || (m_max > 32 && !is(env.lazy, '0')) || small_batch) return plan_lazy(B, d, env, L, complete);
        return plan_group(B, d, m_max <= 32 ? 16 : 32, 2, env, L);
    }
    const int gs = group_size_r(m_max);
    if (d >= 5) {
        // more than 32 rows: one polytope per wavefront, F3 / F2 on the dense engine (round 3: (64,8) B = 5 000 0.657 ->
        // 0.453 ms, (48,6) B = 20 000 1.08 -> 0.80 ms, ahead of the two-rows-per-lane kernel AND of the latency form at every
        // batch size, scripts/debug/wdense_ab.py); and any row count while the batch is small
        const bool small_batch = !env.lazy && B <= PLP_REDUCE_WG_MAXB && !env.split && !env.half;
        if (is(env.lazy, '1') || (m_max > 32 && !is(env.lazy, '0')) || small_batch) return plan_lazy(B, d, env, L, complete);
        // beyond the latency form's batch sizes: two rows per lane (three wavefronts per SIMD instead of two; the kernel is
        // bound by the latency of the pivot's dependency chain here).  Measured (ms per batch, four rows -> two rows per
        // lane): (32,6) B = 20 000 0.561 -> 0.497, (32,8) 0.674 -> 0.566, (24,5) 0.355 -> 0.310, (64,8) B = 5 000 0.721 ->
        // 0.616; a tie once the batch fills the chip either way ((32,6) B = 100 000: 1.99 -> 1.95)
        const bool latency_form = is(env.split, '1') || (!is(env.split, '0') && B <= PLP_REDUCE_SPLIT_MAXB(d, gs));
        if (!latency_form) return plan_group(B, d, m_max <= 16 ? 8 : (m_max <= 32 ? 16 : 32), 2, env, L);
    }
    return plan_group(B, d, gs, 4, env, L);
}

}  // namespace plan_detail

inline ReducePlan plan_reduce(long long B, int m_max, int d, const ReduceEnv& env) {
    using namespace plan_detail;
    ReducePlan p;
    if (m_max < 0 || m_max > 64 || d < 1 || d > 16) return p;
    p.force_retry = is(env.retry_all, '1') ? 1 : 0;
    const int gs = reduce_general_gs(m_max);
    long long blocks = cdiv(B, REDUCE_GENERAL_BLOCK / gs);
    if (blocks > (1ll << 20)) blocks = 1ll << 20;   // one tile per block: the dispatcher balances the tail
    blocks = at_least1(blocks);
    // the second pass mostly reads flags: a grid-stride sweep
    p.retry = launch(RE_GENERAL, gs, 1, blocks > 256 * 8 ? 256 * 8 : blocks, REDUCE_GENERAL_BLOCK, reduce_smem_bytes(gs, d));
    p.first = p.retry;
    p.first.grid = blocks;
    bool complete = false;
    ReduceLaunch fast;
    if (is(env.one_row, '1') || !plan_fast(B, m_max, d, env, fast, complete)) return p;
    p.first = fast;
    p.second = !complete;
    return p;
}

}  // namespace plp
