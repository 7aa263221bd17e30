// plp_locate.hip -- point location (gfx950): first containing polytope per point, and how many contain it.
// No counterpart in the reference (its users loop `x in region` over a partition, one point at a time); the arithmetic
// of one (row, point) test is contains_kernel's (plp_points.hip), restated in plp_locate.hpp.
//
//   locate_dense_kernel<D,PPL,COUNT> : every polytope against every point, laid out like contains_kernel -- PPL points per
//                                      lane in VGPRs, rows wave-uniform through the scalar cache, verdicts as ballot masks
//                                      -- with a per-point `first` (and `count`) in place of the OR.  Polytopes are visited
//                                      in ascending order, so a point's first hit is its answer, and without COUNT the
//                                      wavefront leaves the polytope loop once none of its points is still open.
//   locate_grid_count_kernel / locate_scan_kernel / locate_grid_fill_kernel / locate_sort_kernel :
//                                      the cell lists of the culling grid (plp_locate.hpp): one thread per polytope walks
//                                      its cell range with ordinary vector atomics on per-cell counters and cursors, a
//                                      one-workgroup exclusive scan in between, one thread per cell sorts its list.
//   locate_grid_kernel<D,COUNT>      : one point per lane; the lane walks the list of its cell and tests each candidate
//                                      row by row, leaving a candidate at its first violated row.  Rows differ per lane and
//                                      come through vector loads.  Lanes of a wavefront diverge (different lists, different
//                                      rows at which they leave); NOT MEASURED -- see DESIGN 4.15.
#include "plp_kernels.hpp"
#include "plp_locate.hpp"

namespace plp {

template <int D, int PPL, bool COUNT>
__global__ __launch_bounds__(BLOCK) void locate_dense_kernel(int P, int m_max, const double* __restrict__ A,
                                                             const double* __restrict__ b, const int* __restrict__ mrows,
                                                             long long N, const double* __restrict__ X, double tol,
                                                             int* __restrict__ first, int* __restrict__ count) {
    const long long stride = (long long)gridDim.x * BLOCK;
    const unsigned long long me = 1ull << (threadIdx.x & 63);
    // (the loop variable is the workgroup's first point: every lane of a wavefront makes the same trips, so the ballots
    // below always see the whole wavefront)
    for (long long base = (long long)blockIdx.x * BLOCK; base < N; base += stride * PPL) {
        const long long q0 = base + threadIdx.x;
        double x[PPL][D];
        bool inb[PPL];
        int fst[PPL], cnt[PPL];
        unsigned long long open_m[PPL];  // lanes whose point (in range) has no first yet
#pragma unroll
        for (int t = 0; t < PPL; ++t) {
            const long long q = q0 + t * stride;
            inb[t] = q < N;
#pragma unroll
            for (int k = 0; k < D; ++k) x[t][k] = inb[t] ? X[(long long)k * N + q] : 0.0;
            fst[t] = -1;
            cnt[t] = 0;
            open_m[t] = __ballot(inb[t]);
        }
        for (int p = 0; p < P; ++p) {
            const int m = mrows ? mrows[p] : m_max;
            const double* Ap = A + (size_t)p * m_max * D;
            const double* bp = b + (size_t)p * m_max;
            unsigned long long ok_m[PPL];
#pragma unroll
            for (int t = 0; t < PPL; ++t) ok_m[t] = ~0ull;
            for (int i = 0; i < m; ++i) {  // rows are wave-uniform: scalar loads, SGPR operands
                double ar[D];
#pragma unroll
                for (int k = 0; k < D; ++k) ar[k] = Ap[i * D + k];
                const double bi = bp[i];
#pragma unroll
                for (int t = 0; t < PPL; ++t) {
                    double s = ar[0] * x[t][0];
#pragma unroll
                    for (int k = 1; k < D; ++k) s = fma(ar[k], x[t][k], s);
                    ok_m[t] &= __ballot((s - bi) < tol);
                }
            }
            unsigned long long still = 0ull;
#pragma unroll
            for (int t = 0; t < PPL; ++t) {
                if (ok_m[t] & open_m[t] & me) fst[t] = p;
                open_m[t] &= ~ok_m[t];
                still |= open_m[t];
                if constexpr (COUNT) cnt[t] += (ok_m[t] & me) ? 1 : 0;
            }
            if constexpr (!COUNT) {
                if (!still) break;  // (scalar: every open point of the wavefront has its answer)
            }
        }
#pragma unroll
        for (int t = 0; t < PPL; ++t) {
            const long long q = q0 + t * stride;
            if (inb[t]) {
                first[q] = fst[t];
                if constexpr (COUNT) count[q] = cnt[t];
            }
        }
    }
}

template <int D, bool COUNT>
__global__ __launch_bounds__(BLOCK) void locate_grid_kernel(int P, int m_max, const double* __restrict__ A,
                                                            const double* __restrict__ b, const int* __restrict__ mrows,
                                                            long long N, const double* __restrict__ X, double tol,
                                                            const loc::Grid g, const int* __restrict__ cell_start,
                                                            const int* __restrict__ cell_items, int* __restrict__ first,
                                                            int* __restrict__ count) {
    const long long stride = (long long)gridDim.x * BLOCK;
    for (long long q = (long long)blockIdx.x * BLOCK + threadIdx.x; q < N; q += stride) {
        double x[D];
#pragma unroll
        for (int k = 0; k < D; ++k) x[k] = X[(long long)k * N + q];
        // (the gridded coordinates are read from X again, by axis number: indexing x[] with it would put x in scratch)
        const int c = loc::point_cell(g, X + q, N);
        const int t1 = cell_start[c + 1];
        int fst = -1, cnt = 0;
        for (int t = cell_start[c]; t < t1; ++t) {
            const int p = cell_items[t];
            if ((unsigned)p >= (unsigned)P) continue;  // (lists of another table: never read rows out of bounds)
            const int m = mrows ? mrows[p] : m_max;
            const double* Ap = A + (size_t)p * m_max * D;
            const double* bp = b + (size_t)p * m_max;
            bool in = true;
            for (int i = 0; i < m && in; ++i) in = loc::row_inside<D>(Ap + i * D, bp[i], x, tol);
            if (in) {
                if (fst < 0) fst = p;
                if constexpr (COUNT) ++cnt;
                else break;  // lists are ascending: the first hit is the answer
            }
        }
        first[q] = fst;
        if constexpr (COUNT) count[q] = cnt;
    }
}

// cell_start[1 + c] += 1 for every cell c of every polytope's range (cell_start zeroed by the launcher)
__global__ __launch_bounds__(BLOCK) void locate_grid_count_kernel(int P, int d, const double* __restrict__ lb,
                                                                  const double* __restrict__ ub, double pad, const loc::Grid g,
                                                                  int* __restrict__ cell_start) {
    const int p = blockIdx.x * BLOCK + threadIdx.x;
    if (p >= P) return;
    int lo[loc::MAX_AXES], hi[loc::MAX_AXES];
    if (!loc::cell_range(g, d, lb + (size_t)p * d, ub + (size_t)p * d, pad, lo, hi)) return;
    loc::for_cells(g, lo, hi, [&](int c) { atomicAdd(&cell_start[c + 1], 1); });
}

// one workgroup: cell_start[1 .. G] (list lengths) -> inclusive prefix sums in place, i.e. with cell_start[0] = 0 the
// exclusive starts; sums saturate at 2^31 - 1 (such a grid is declined by the caller); *max_len = the longest list
constexpr int SCAN_T = 1024;
__global__ __launch_bounds__(SCAN_T) void locate_scan_kernel(int G, int* __restrict__ cell_start, int* __restrict__ max_len) {
    __shared__ long long ssum[SCAN_T];
    __shared__ int smax[SCAN_T];
    const int tid = threadIdx.x;
    const int per = (G + SCAN_T - 1) / SCAN_T;
    const int c0 = tid * per < G ? tid * per : G;
    const int c1 = c0 + per < G ? c0 + per : G;
    long long sum = 0;
    int mx = 0;
    for (int c = c0; c < c1; ++c) {
        const int n = cell_start[1 + c];
        sum += n;
        mx = n > mx ? n : mx;
    }
    ssum[tid] = sum;
    smax[tid] = mx;
    __syncthreads();
    for (int off = 1; off < SCAN_T; off <<= 1) {
        const long long v = tid >= off ? ssum[tid - off] : 0;
        const int w = tid >= off ? smax[tid - off] : 0;
        __syncthreads();
        ssum[tid] += v;
        smax[tid] = w > smax[tid] ? w : smax[tid];
        __syncthreads();
    }
    long long run = ssum[tid] - sum;
    for (int c = c0; c < c1; ++c) {
        run += cell_start[1 + c];
        cell_start[1 + c] = run > 2147483647ll ? 2147483647 : (int)run;
    }
    if (tid == 0) cell_start[0] = 0;
    if (tid == SCAN_T - 1) *max_len = smax[tid];
}

// cell_items[cell_start[c] + k] = p, k the order of arrival (cursor zeroed by the launcher)
__global__ __launch_bounds__(BLOCK) void locate_grid_fill_kernel(int P, int d, const double* __restrict__ lb,
                                                                 const double* __restrict__ ub, double pad, const loc::Grid g,
                                                                 const int* __restrict__ cell_start, int* __restrict__ cursor,
                                                                 int* __restrict__ cell_items) {
    const int p = blockIdx.x * BLOCK + threadIdx.x;
    if (p >= P) return;
    int lo[loc::MAX_AXES], hi[loc::MAX_AXES];
    if (!loc::cell_range(g, d, lb + (size_t)p * d, ub + (size_t)p * d, pad, lo, hi)) return;
    loc::for_cells(g, lo, hi, [&](int c) {
        const int pos = cell_start[c] + atomicAdd(&cursor[c], 1);
        if (pos < cell_start[c + 1]) cell_items[pos] = p;  // (always, when cell_start is the count pass of the same boxes)
    });
}

// every cell's list ascending: one thread per cell, insertion sort (lists are short; the caller caps them)
__global__ __launch_bounds__(BLOCK) void locate_sort_kernel(int G, const int* __restrict__ cell_start, int* __restrict__ cell_items) {
    const int c = blockIdx.x * BLOCK + threadIdx.x;
    if (c >= G) return;
    const int t0 = cell_start[c], t1 = cell_start[c + 1];
    for (int t = t0 + 1; t < t1; ++t) {
        const int v = cell_items[t];
        int u = t - 1;
        while (u >= t0 && cell_items[u] > v) { cell_items[u + 1] = cell_items[u]; --u; }
        cell_items[u + 1] = v;
    }
}

__global__ __launch_bounds__(BLOCK) void locate_none_kernel(long long N, int* __restrict__ first, int* __restrict__ count) {
    const long long stride = (long long)gridDim.x * BLOCK;
    for (long long q = (long long)blockIdx.x * BLOCK + threadIdx.x; q < N; q += stride) {
        first[q] = -1;
        if (count) count[q] = 0;
    }
}

static unsigned point_blocks(long long N, int ppl) {
    long long blocks = (N + (long long)BLOCK * ppl - 1) / ((long long)BLOCK * ppl);
    if (blocks > 256ll * 32) blocks = 256ll * 32;
    return (unsigned)(blocks < 1 ? 1 : blocks);
}

template <int D>
static void launch_locate_d(int P, int m_max, const double* A, const double* b, const int* mrows, long long N,
                            const double* X, double tol, const loc::Grid* g, const int* cell_start, const int* cell_items,
                            int* first, int* count, hipStream_t st) {
    if (g) {
        const unsigned blocks = point_blocks(N, 1);
        if (count)
            hipLaunchKernelGGL((locate_grid_kernel<D, true>), dim3(blocks), dim3(BLOCK), 0, st, P, m_max, A, b, mrows, N, X, tol,
                               *g, cell_start, cell_items, first, count);
        else
            hipLaunchKernelGGL((locate_grid_kernel<D, false>), dim3(blocks), dim3(BLOCK), 0, st, P, m_max, A, b, mrows, N, X, tol,
                               *g, cell_start, cell_items, first, count);
        return;
    }
    // points per lane: contains_kernel's table (plp_points.hip: measured there; NOT measured for this kernel)
    constexpr int PPL = (D <= 3) ? 8 : ((D <= 8) ? 6 : (D == 9 ? 4 : (D <= 12 ? 3 : 2)));
    const unsigned blocks = point_blocks(N, PPL);
    if (count)
        hipLaunchKernelGGL((locate_dense_kernel<D, PPL, true>), dim3(blocks), dim3(BLOCK), 0, st, P, m_max, A, b, mrows, N, X,
                           tol, first, count);
    else
        hipLaunchKernelGGL((locate_dense_kernel<D, PPL, false>), dim3(blocks), dim3(BLOCK), 0, st, P, m_max, A, b, mrows, N, X,
                           tol, first, count);
}

#define PLP_CASE_L(K) case K: launch_locate_d<K>(P, m_max, A, b, mrows, N, X, abs_tol, grid, cell_start, cell_items, first, count, st); break;

int launch_locate(int P, int m_max, int d, const double* A, const double* b, const int* mrows, long long N, const double* X,
                  double abs_tol, const plp_locate_grid* grid, const int* cell_start, const int* cell_items, int* first,
                  int* count, hipStream_t st) {
    if (d < 1 || d > MAX_D || m_max < 0 || P < 0 || N < 0) return 2;
    if (grid && loc::grid_bad(*grid, d)) return 2;
    if (N == 0) return 0;
    if (P == 0) {
        hipLaunchKernelGGL(locate_none_kernel, dim3(point_blocks(N, 1)), dim3(BLOCK), 0, st, N, first, count);
        return 0;
    }
    switch (d) {
        PLP_CASE_L(1) PLP_CASE_L(2) PLP_CASE_L(3) PLP_CASE_L(4) PLP_CASE_L(5) PLP_CASE_L(6)
        PLP_CASE_L(7) PLP_CASE_L(8) PLP_CASE_L(9) PLP_CASE_L(10) PLP_CASE_L(11) PLP_CASE_L(12)
        PLP_CASE_L(13) PLP_CASE_L(14) PLP_CASE_L(15) PLP_CASE_L(16)
        default: return 2;
    }
    return 0;
}

int launch_locate_grid_count(int P, int d, const double* lb, const double* ub, double pad, const plp_locate_grid* grid,
                             int* cell_start, int* max_len, hipStream_t st) {
    if (d < 1 || d > MAX_D || P < 0 || !grid || loc::grid_bad(*grid, d) || !(pad >= 0.0)) return 2;
    const int G = loc::n_cells(*grid);
    if (hipMemsetAsync(cell_start, 0, ((size_t)G + 1) * sizeof(int), st) != hipSuccess) return 3;
    if (P > 0)
        hipLaunchKernelGGL(locate_grid_count_kernel, dim3((unsigned)((P + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, st, P, d, lb, ub,
                           pad, *grid, cell_start);
    hipLaunchKernelGGL(locate_scan_kernel, dim3(1), dim3(SCAN_T), 0, st, G, cell_start, max_len);
    return 0;
}

int launch_locate_grid_fill(int P, int d, const double* lb, const double* ub, double pad, const plp_locate_grid* grid,
                            const int* cell_start, int* cursor, int* cell_items, hipStream_t st) {
    if (d < 1 || d > MAX_D || P < 0 || !grid || loc::grid_bad(*grid, d) || !(pad >= 0.0)) return 2;
    if (P == 0) return 0;
    const int G = loc::n_cells(*grid);
    if (hipMemsetAsync(cursor, 0, (size_t)G * sizeof(int), st) != hipSuccess) return 3;
    hipLaunchKernelGGL(locate_grid_fill_kernel, dim3((unsigned)((P + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, st, P, d, lb, ub, pad,
                       *grid, cell_start, cursor, cell_items);
    hipLaunchKernelGGL(locate_sort_kernel, dim3((unsigned)((G + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, st, G, cell_start,
                       cell_items);
    return 0;
}

}  // namespace plp
