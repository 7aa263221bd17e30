// plp_box_pairs.hip -- the broad phase of the sparse pair calls (gfx950): the pairs of cells whose padded outer boxes meet
// (the rule, its grid form and why the cull is exact: plp_box_pairs.hpp).  No counterpart in the reference, which tests
// every pair (prop2partition.py:57-61).
//
//   box_pairs_kernel<FILL> : ONE WAVEFRONT PER CELL i.  The cell's own box, its cell range and its partner range are
//                            wave-uniform (scalar loads); the lanes stride over what the cell meets, one entry per lane, a
//                            ballot counts the hits of the 64 and gives each its slot.  Partner counts per cell differ by
//                            orders of magnitude (a slab or a half-space meets every cell), and a cell per lane would leave
//                            a wavefront waiting for its longest list; here every wavefront works at the width of its list.
//                            Two walks, the same set (plp_box_pairs.hpp):
//                              brute -- the lanes stride over the partner range [j_lo, j_hi): every partner is box-tested.
//                                       Partners are met ascending, so the slots are the output order.
//                              grid  -- the wavefront walks the grid cells of its range, the lanes stride over each
//                                       list, and a pair counts in its canonical cell only.  Partners come in walk order:
//                                       FILL collects them in LDS and writes each at its rank (they are distinct).
//                            Which walk a cell takes decides speed only: the grid walk when its range holds at most half as
//                            many grid cells as the brute walk has steps (PLP_BOX_WALK=0 / 1: never / always -- A/B, tests),
//                            and in FILL only for up to BP_WALK_MAX partners (the LDS buffer; beyond, the brute walk, whose
//                            cost does not grow with the list).  COUNT writes the cell's number of partners, FILL the
//                            pairs (i, j) at per_cell[i] - per_cell[cell_lo] on.
//   box_pairs_scan_kernel  : one workgroup, counts -> exclusive prefix sums (int64), as locate_scan_kernel.
// NOT MEASURED -- see DESIGN 4.20.
#include "plp_box_pairs.hpp"
#include "plp_kernels.hpp"

namespace plp {

constexpr int BP_WALK_MAX = 1024;

template <bool FILL>
__global__ __launch_bounds__(64) void box_pairs_kernel(int n, int d, const double* __restrict__ lb, const double* __restrict__ ub,
                                                       double pad, int use_grid, const loc::Grid g,
                                                       const int* __restrict__ cell_start, const int* __restrict__ cell_items,
                                                       int n1, int walk_mode, int cell_lo, long long* __restrict__ counts,
                                                       const long long* __restrict__ per_cell, int* __restrict__ pairs) {
    __shared__ int buf[FILL ? BP_WALK_MAX : 1];
    const int i = cell_lo + (int)blockIdx.x;  // (the launcher's grid is cell_hi - cell_lo: i < n)
    const int lane = threadIdx.x;
    const unsigned long long below = (1ull << lane) - 1ull;
    long long base = 0, L = 0;
    if constexpr (FILL) {
        base = per_cell[i] - per_cell[cell_lo];
        L = per_cell[i + 1] - per_cell[i];
        if (L <= 0) return;
    }
    int j_lo, j_hi;
    bp::partner_range(n, n1, i, &j_lo, &j_hi);
    const double* lbi = lb + (size_t)i * d;
    const double* ubi = ub + (size_t)i * d;
    int lo[loc::MAX_AXES] = {0, 0, 0}, hi[loc::MAX_AXES] = {0, 0, 0};
    bool none = j_lo >= j_hi, walk = false;
    if (use_grid && !none) {
        // (listed nowhere: the padded box is empty on a gridded axis, and the rule pairs such a cell with nothing)
        none = !loc::cell_range(g, d, lbi, ubi, pad, lo, hi);
        const long long cells = (long long)(hi[0] - lo[0] + 1) * (hi[1] - lo[1] + 1) * (hi[2] - lo[2] + 1);
        const long long steps = ((long long)j_hi - j_lo + 63) / 64;
        walk = walk_mode == 1 || (walk_mode != 0 && 2 * cells <= steps);
        if (FILL && L > BP_WALK_MAX) walk = false;
    }
    if (none) {
        if (!FILL && lane == 0) counts[i] = 0;
        return;
    }
    const double ps_i = pad * bp::box_scale(d, lbi, ubi);
    long long cnt = 0;  // wave-uniform: the partners found so far
    if (walk) {
        const int r1 = g.naxes > 1 ? g.res[1] : 1, r2 = g.naxes > 2 ? g.res[2] : 1;
        for (int c0 = lo[0]; c0 <= hi[0]; ++c0)
            for (int c1 = lo[1]; c1 <= hi[1]; ++c1)
                for (int c2 = lo[2]; c2 <= hi[2]; ++c2) {
                    int c = c0;
                    if (g.naxes > 1) c = c * r1 + c1;
                    if (g.naxes > 2) c = c * r2 + c2;
                    const int t1 = cell_start[c + 1];
                    for (int tb = cell_start[c]; tb < t1; tb += 64) {
                        const int t = tb + lane;
                        int j = -1;
                        bool hit = false;
                        if (t < t1) {
                            j = cell_items[t];
                            // (lists of another table: never read boxes out of bounds)
                            hit = (unsigned)j < (unsigned)n && bp::walk_hit(g, d, lb, ub, pad, i, lo, ps_i, j, j_lo, j_hi, c0, c1, c2);
                        }
                        const unsigned long long mask = __ballot(hit);
                        if constexpr (FILL) {
                            const long long pos = cnt + __popcll(mask & below);
                            if (hit && pos < L) buf[pos] = j;
                        }
                        cnt += __popcll(mask);
                    }
                }
        if constexpr (FILL) {
            __syncthreads();
            const int Ls = (int)(cnt < L ? cnt : L);
            for (int e = lane; e < Ls; e += 64) {
                const int v = buf[e];
                int r = 0;
                for (int t = 0; t < Ls; ++t) r += buf[t] < v ? 1 : 0;
                pairs[2 * (base + r)] = i;
                pairs[2 * (base + r) + 1] = v;
            }
        }
    } else {
        for (long long jb = j_lo; jb < j_hi; jb += 64) {
            const long long j = jb + lane;
            bool hit = false;
            if (j < j_hi) {
                const double* lbj = lb + (size_t)j * d;
                const double* ubj = ub + (size_t)j * d;
                hit = bp::boxes_meet(d, lbi, ubi, ps_i, lbj, ubj, pad * bp::box_scale(d, lbj, ubj));
            }
            const unsigned long long mask = __ballot(hit);
            if constexpr (FILL) {
                const long long pos = cnt + __popcll(mask & below);
                if (hit && pos < L) {
                    pairs[2 * (base + pos)] = i;
                    pairs[2 * (base + pos) + 1] = (int)j;
                }
            }
            cnt += __popcll(mask);
        }
    }
    if (!FILL && lane == 0) counts[i] = cnt;
}

// one workgroup: per_cell[1 .. n] (partner counts) -> inclusive prefix sums in place, i.e. with per_cell[0] = 0 the
// exclusive starts
constexpr int BP_SCAN_T = 1024;
__global__ __launch_bounds__(BP_SCAN_T) void box_pairs_scan_kernel(int n, long long* __restrict__ per_cell) {
    __shared__ long long ssum[BP_SCAN_T];
    const int tid = threadIdx.x;
    const int per = (n + BP_SCAN_T - 1) / BP_SCAN_T;
    const long long c0 = (long long)tid * per < n ? (long long)tid * per : n;
    const long long c1 = c0 + per < n ? c0 + per : n;
    long long sum = 0;
    for (long long c = c0; c < c1; ++c) sum += per_cell[1 + c];
    ssum[tid] = sum;
    __syncthreads();
    for (int off = 1; off < BP_SCAN_T; off <<= 1) {
        const long long v = tid >= off ? ssum[tid - off] : 0;
        __syncthreads();
        ssum[tid] += v;
        __syncthreads();
    }
    long long run = ssum[tid] - sum;
    for (long long c = c0; c < c1; ++c) {
        run += per_cell[1 + c];
        per_cell[1 + c] = run;
    }
    if (tid == 0) per_cell[0] = 0;
}

static int walk_mode() {
    const char* e = getenv("PLP_BOX_WALK");  // read per call (tests change it between the calls of one process)
    return (e && e[0] == '0') ? 0 : ((e && e[0] == '1') ? 1 : -1);
}

static bool box_pairs_bad(int n, int d, double pad, const plp_locate_grid* grid, int n1) {
    return d < 1 || d > MAX_D || n < 0 || n1 < 0 || n1 > n || !(pad >= 0.0) || (grid && loc::grid_bad(*grid, d));
}

int launch_box_pairs_count(int n, int d, const double* lb, const double* ub, double pad, const plp_locate_grid* grid,
                           const int* cell_start, const int* cell_items, int n1, long long* per_cell, hipStream_t st) {
    if (box_pairs_bad(n, d, pad, grid, n1)) return 2;
    if (n == 0) return hipMemsetAsync(per_cell, 0, sizeof(long long), st) == hipSuccess ? 0 : 3;
    const loc::Grid g = grid ? *grid : loc::Grid{};
    hipLaunchKernelGGL((box_pairs_kernel<false>), dim3((unsigned)n), dim3(64), 0, st, n, d, lb, ub, pad, grid ? 1 : 0, g, cell_start,
                       cell_items, n1, walk_mode(), 0, per_cell + 1, (const long long*)nullptr, (int*)nullptr);
    hipLaunchKernelGGL(box_pairs_scan_kernel, dim3(1), dim3(BP_SCAN_T), 0, st, n, per_cell);
    return 0;
}

int launch_box_pairs_fill(int n, int d, const double* lb, const double* ub, double pad, const plp_locate_grid* grid,
                          const int* cell_start, const int* cell_items, int n1, const long long* per_cell, int cell_lo,
                          int cell_hi, int* pairs, hipStream_t st) {
    if (box_pairs_bad(n, d, pad, grid, n1) || cell_lo < 0 || cell_hi > n || cell_lo > cell_hi) return 2;
    if (cell_lo == cell_hi) return 0;
    const loc::Grid g = grid ? *grid : loc::Grid{};
    hipLaunchKernelGGL((box_pairs_kernel<true>), dim3((unsigned)(cell_hi - cell_lo)), dim3(64), 0, st, n, d, lb, ub, pad,
                       grid ? 1 : 0, g, cell_start, cell_items, n1, walk_mode(), cell_lo, (long long*)nullptr, per_cell, pairs);
    return 0;
}

}  // namespace plp
