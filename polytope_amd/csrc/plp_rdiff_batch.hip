// plp_rdiff_batch.hip -- rdiff_batch_kernel<D>: B set differences (a polytope minus an ordered list of cells) in one launch,
// one whole search per wavefront (plp_rdiff_batch.hpp: the contract, the caps, the sequential rule).  No mailbox, no host
// round trip, no resident kernel: the table of a problem sits in LDS, lane 0 walks the search on a State in LDS and every
// Chebyshev LP it asks for is solved by the wavefront on the one-LP-per-wavefront engine (plp_wide.hpp).
#include "plp_kernels.hpp"
#include "plp_rdiff_batch.hpp"
#include "plp_wide.hpp"

namespace plp {

// Workgroup (= wavefront) P, P + grid, ... takes problem P.
//   stage : lane i < m puts minuend row i into the table T[m + M][D + 1] (the M negations are formed on reading)
//   build : cell after cell of the problem's list, lane r holds row r of the cell and compares it with all minuend rows
//           (every lane reads the same LDS address: a broadcast); the new rows are appended in row order
//   search: lane 0 runs rdb::step() up to the next radius it reads; lane i fetches row i of that list from T; the
//           wavefront solves the LP; the radius goes back into step().  Every LP counts against max_lps.
// Only rows < m[P] of a minuend and rows < mc[c] of a LISTED cell are read.
// cell_off must be non-decreasing from a cell_off[0] >= 0 and end within cell_idx, whose length the kernel is not told: a
// negative or decreasing entry ends that problem as RD_UNSUPPORTED, an entry past the end of cell_idx is the caller's.
template <int D>
__global__ __launch_bounds__(64) void rdiff_batch_kernel(
    const long long B, const int m_max, const double* __restrict__ Ag, const double* __restrict__ bg,
    const int* __restrict__ mrows, const long long Nc, const int mc_max, const double* __restrict__ CAg,
    const double* __restrict__ Cbg, const int* __restrict__ mcg, const int* __restrict__ cell_off,
    const int* __restrict__ cell_idx, const double abs_tol, const int max_lps, const int p_max, const int r_max,
    const int n_max, const int M_max, int* __restrict__ kind, int* __restrict__ off, int* __restrict__ rows,
    int* __restrict__ count, int* __restrict__ nrows, int* __restrict__ nlp, int* __restrict__ status,
    int* __restrict__ mi_out, int* __restrict__ src) {
    constexpr int D1 = D + 1;
    __shared__ rdb::State s;
    __shared__ double T[rdb::MAX_STORED * D1];
    __shared__ wide::WideShared<D1> sh;
    __shared__ int act;
    const int lane = threadIdx.x;
    for (long long P = blockIdx.x; P < B; P += gridDim.x) {
        __syncthreads();   // (the last problem's reads of the block are done)
        int m = mrows ? mrows[P] : m_max;
        m = m < 0 ? 0 : (m > m_max ? m_max : m);
        const long long c0 = cell_off[P];
        const long long Nl = (long long)cell_off[P + 1] - c0;
        const int N = Nl < 0 ? -1 : (Nl > rdb::MAX_CELLS ? rdb::MAX_CELLS + 1 : (int)Nl);
        int st = c0 < 0 ? (int)rdb::RD_UNSUPPORTED : rdb::check_shape(m, N);   // (N < 0: cell_off decreases here)
        const rdb::Out o{kind + P * p_max, off + P * (p_max + 1), rows + P * r_max, p_max, r_max};
        int M = 0;
        bool covered = false;
        if (st == rdb::RD_OK) {
            if (lane < m) {
                const long long g = P * m_max + lane;
#pragma unroll
                for (int k = 0; k < D; ++k) T[lane * D1 + k] = Ag[g * D + k];
                T[lane * D1 + D] = bg[g];
            }
            __syncthreads();
            for (int j = 0; j < N && st == rdb::RD_OK; ++j) {
                const long long c = cell_idx[c0 + j];
                if (c < 0 || c >= Nc) {
                    st = rdb::RD_UNSUPPORTED;
                    break;
                }
                int mcj = mcg ? mcg[c] : mc_max;
                mcj = mcj < 0 ? 0 : (mcj > mc_max ? mc_max : mcj);
                double row[D1];
#pragma unroll
                for (int k = 0; k < D1; ++k) row[k] = 0.0;
                bool is_new = false;
                if (lane < mcj && mcj <= rdb::MAX_LIST) {
                    const long long g = c * mc_max + lane;
#pragma unroll
                    for (int k = 0; k < D; ++k) row[k] = CAg[g * D + k];
                    row[D] = Cbg[g];
                    is_new = rdb::row_is_new<D>(row, T, m, abs_tol);
                }
                const unsigned long long nb = __ballot(is_new);
                const int cnt = __popcll(nb);
                if (!rdb::cell_fits(m, M, cnt, mcj)) {
                    st = rdb::RD_UNSUPPORTED;
                    break;
                }
                if (is_new) {
                    const int pos = M + __popcll(nb & ((1ull << lane) - 1ull));
#pragma unroll
                    for (int k = 0; k < D1; ++k) T[(m + pos) * D1 + k] = row[k];
                    if (pos < M_max) src[P * M_max + pos] = (int)(c * mc_max + lane);
                }
                if (lane == 0) {
                    s.mi[j] = cnt;
                    if (j < n_max) mi_out[P * n_max + j] = cnt;
                }
                covered = covered || cnt == 0;
                M += cnt;
            }
        }
        if (st == rdb::RD_OK && covered) st = rdb::RD_COVERED;
        if (lane == 0) {
            o.off[0] = 0;
            if (st == rdb::RD_OK) {
                s.m = m;
                s.N = N;
                rdb::init(s);
            }
        }
        __syncthreads();
        if (st != rdb::RD_OK) {
            if (lane == 0) {
                count[P] = 0;
                nrows[P] = 0;
                nlp[P] = 0;
                status[P] = st;
            }
            continue;
        }
        double R = 0.0;
        for (;;) {
            if (lane == 0) act = rdb::step(s, o, abs_tol, max_lps, R);
            __syncthreads();
            if (act != rdb::ACT_LP) break;
            const int ncur = s.ncur, n = ncur + s.suf_n;
            const bool has = lane < n;
            double a[D], bi = 0.0;
#pragma unroll
            for (int k = 0; k < D; ++k) a[k] = 0.0;
            if (has) {
                const int r = lane < ncur ? s.cur[lane] : s.suf_beg + (lane - ncur);
                const bool neg = r >= m + M;
                const double* src_row = T + (neg ? r - M : r) * D1;
#pragma unroll
                for (int k = 0; k < D; ++k) a[k] = neg ? -src_row[k] : src_row[k];
                bi = neg ? -src_row[D] : src_row[D];
            }
            R = wide::cheby_radius_rows<D>(lane, n, has, a, bi, sh);
            __syncthreads();   // (the list has been read: lane 0 may move on)
        }
        if (lane == 0) {
            count[P] = s.count;
            nrows[P] = s.nout;
            nlp[P] = s.nlp;
            status[P] = s.status;
        }
    }
}

// 0 when launched, 2 for a size the kernel does not take
int launch_rdiff_batch(long long B, int m_max, int d, const double* A, const double* b, const int* m, long long Nc, int mc_max,
                       const double* CA, const double* Cb, const int* mc, const int* cell_off, const int* cell_idx,
                       double abs_tol, int max_lps, int p_max, int r_max, int n_max, int M_max, int* kind, int* off, int* rows,
                       int* count, int* nrows, int* nlp, int* status, int* mi, int* src, hipStream_t st) {
    if (B < 1 || B > 2147483647ll || m_max < 0 || mc_max < 0 || p_max < 1 || r_max < 1 || n_max < 0 || M_max < 0) return 2;
    if (d < 1 || d > rdb::MAX_DIM) return 2;
    // a fixed grid striding over B: enough workgroups of one wavefront to fill the device several times over
    const long long cap = 1ll << 16;
    const unsigned grid = (unsigned)(B < cap ? B : cap);
#define PLP_RDB(K)                                                                                                         \
    case K:                                                                                                                \
        hipLaunchKernelGGL((rdiff_batch_kernel<K>), dim3(grid), dim3(64), 0, st, B, m_max, A, b, m, Nc, mc_max, CA, Cb, mc, \
                           cell_off, cell_idx, abs_tol, max_lps, p_max, r_max, n_max, M_max, kind, off, rows, count, nrows,  \
                           nlp, status, mi, src);                                                                          \
        return 0;
    switch (d) {
        PLP_RDB(1) PLP_RDB(2) PLP_RDB(3) PLP_RDB(4)
        default: return 2;
    }
#undef PLP_RDB
}

}  // namespace plp
