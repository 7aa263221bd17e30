// plp_wide.hip -- one LP per WAVEFRONT, one dictionary row per lane, for the large shapes (d = 9..16, m <= 64).
//
//   cheby_w_kernel<D> : Chebyshev-ball LPs (form F1, polytope/polytope.py:1283-1288) of a batch of polytopes
//
// The lane-group engines (plp_simplex.hpp, plp_simplex_r.hpp) let several LPs share a wavefront, so the entering
// column differs from lane to lane and every access T[e] is a chain of selects over the columns: at 17 columns that
// chain (and its twin for the column fix-up) is most of the ~500 VALU instructions a (64,17) pivot costs there.  Here a
// wavefront owns ONE LP: the entering column e and the pivot row r are wave-uniform (SGPRs), so
//   * T[e] is one indexed register move (the row is a register vector), not 17 selects;
//   * the reduced costs live ONCE, in LDS, lane j looking after column j: pricing is one load, one compare and a
//     DPP wave reduction instead of a 17-step scan of replicated values, and the cost row's update is one FMA;
//   * the pivot row is scaled in place by its own lane (exec = that lane), stored to LDS, and read back by all lanes
//     as broadcast ds_reads -- no ds_bpermute pairs, no VALU slots spent on moving it;
//   * the ratio test's exact f64 minimum is a DPP reduction over the 64 lanes (row_bcast15/31 for the upper levels).
// About 110 VALU instructions per pivot.  Pivot rules as everywhere (oracle/plp_oracle.c restates them): free
// variables enter in either direction and never leave, Dantzig pricing (largest |c_j|, lowest column on ties), ratio
// test ties to the lowest row, Bland's rule after BLAND_AFTER consecutive degenerate pivots, forced first pivot
// "r enters, row argmin b_i/||a_i|| leaves" for F1.
#include <stdlib.h>

#include "plp_lp_launch.hpp"
#include "plp_pair_index.hpp"
#include "plp_wave.hpp"
#include "plp_wide.hpp"

namespace plp {

using namespace wide;

template <int D>
__global__ __launch_bounds__(64) void cheby_w_kernel(long long B, int m_max, const double* __restrict__ A,
                                                     const double* __restrict__ b, const int* __restrict__ mrows,
                                                     double* __restrict__ r_out, double* __restrict__ xc,
                                                     int* __restrict__ status) {
    constexpr int NC = D + 1;
    __shared__ WideShared<NC> sh;
    const int lane = threadIdx.x;
    const long long p = blockIdx.x;
    if (p >= B) return;
    const int m = mrows ? mrows[p] : m_max;
    const bool has = lane < m;
    typename RowVec<NC>::type Tv;
    double T16;
    ChebyRow c;
    cheby_setup<D>(Tv, T16, c, lane, has, [&](int k) { return A[(p * m_max + lane) * D + k]; },
                   [&]() { return b[p * m_max + lane]; }, sh);
    __syncthreads();
    const int st = cheby_run<D>(Tv, T16, c, lane, m, sh, m > 64);
    const double qnan = __longlong_as_double(0x7ff8000000000000ll);
#pragma unroll
    for (int j = 0; j < NC; ++j) {
        const double xj = (st == ST_OPT) ? cheby_x(c, j) : qnan;
        if (lane == 0) {
            if (j < D) xc[p * D + j] = xj; else r_out[p] = xj;
        }
    }
    if (lane == 0) status[p] = st;
}

// The same LP on a ROW SUBSET of one resident table (region_diff's search, plp_rdiff.hip): LP q of the class is list
// sel[q] of the batch, its rows rows[off[p] .. off[p + 1]) (at most 64).  out[p] as cheby_gather_r_kernel writes it: the
// radius if the LP is optimal with r >= 0, 0 if optimal with r < 0, NaN for any other status.
template <int D>
__global__ __launch_bounds__(64) void cheby_gather_w_kernel(long long nlp, const int* __restrict__ off,
                                                            const int* __restrict__ rows, const int* __restrict__ sel,
                                                            const double* __restrict__ A, const double* __restrict__ b,
                                                            double* __restrict__ out) {
    constexpr int NC = D + 1;
    __shared__ WideShared<NC> sh;
    const int lane = threadIdx.x;
    const long long q = blockIdx.x;
    if (q >= nlp) return;
    const int p = sel[q];
    const int o = off[p];
    const int m = off[p + 1] - o;
    const bool has = lane < m;
    const long long row = has ? rows[o + lane] : 0;
    typename RowVec<NC>::type Tv;
    double T16;
    ChebyRow c;
    cheby_setup<D>(Tv, T16, c, lane, has, [&](int k) { return A[row * D + k]; }, [&]() { return b[row]; }, sh);
    __syncthreads();
    const int st = cheby_run<D>(Tv, T16, c, lane, m, sh, m > 64);
    const double r = cheby_radius<D>(c);
    if (lane == 0) out[p] = st != ST_OPT ? __builtin_nan("") : (r >= 0.0 ? r : 0.0);
}

template <int D>
static int launch_cheby_gather_w_d(long long nlp, const int* off, const int* rows, const int* sel, const double* A,
                                   const double* b, double* out, hipStream_t st) {
    if (nlp > 2147483647ll) return 2;
    if (nlp < 1) return 0;
    hipLaunchKernelGGL((cheby_gather_w_kernel<D>), dim3((unsigned)nlp), dim3(64), 0, st, nlp, off, rows, sel, A, b, out);
    return 0;
}

#define PLP_CASE_GW(K) case K: return launch_cheby_gather_w_d<K>(nlp, off, rows, sel, A, b, out, st);

// lists of at most 64 rows, d = 5..16; returns 1 when it does not apply
int launch_cheby_gather_w(int d, long long nlp, const int* off, const int* rows, const int* sel, const double* A,
                          const double* b, double* out, hipStream_t st) {
    switch (d) {
        PLP_CASE_GW(2) PLP_CASE_GW(3) PLP_CASE_GW(4)
        PLP_CASE_GW(5) PLP_CASE_GW(6) PLP_CASE_GW(7) PLP_CASE_GW(8) PLP_CASE_GW(9) PLP_CASE_GW(10)
        PLP_CASE_GW(11) PLP_CASE_GW(12) PLP_CASE_GW(13) PLP_CASE_GW(14) PLP_CASE_GW(15) PLP_CASE_GW(16)
        default: return 1;
    }
}

// Pair LPs of find_adjacent_regions / is_adjacent(overlap = True) (polytope/polytope.py:1843-1866 under the pair loop of
// prop2partition.py:57-61), one pair per wavefront: the rows of cell i and of cell j stacked (at most 64), every b
// inflated, adjacent iff the Chebyshev radius exceeds `thresh` -- the contract of adjacent_r_kernel (plp_cheby_r_impl.hpp),
// for d = 5..16 (the lane-group kernel stops at d = 8 and holds one or two such LPs per wavefront from 33 rows on).
// `list` (LISTED, plp_pair_list): pair t of the launch is (list[2 t], list[2 t + 1]), verdicts go to compact[t].
template <int D, bool LISTED>
__device__ __forceinline__ void adjacent_w_body(int n, int m_max, const double* __restrict__ A,
                                                const double* __restrict__ b, const int* __restrict__ mrows,
                                                double inflate, double thresh, unsigned char* __restrict__ adj,
                                                long long p_lo, long long p_hi, unsigned char* __restrict__ compact,
                                                int cross_n1, int mark, const int* __restrict__ list) {
    constexpr int NC = D + 1;
    __shared__ WideShared<NC> sh;
    const int lane = threadIdx.x;
    if (!compact) {  // diagonal
        const long long t = (long long)blockIdx.x * 64 + lane;
        if (t < n) adj[t * n + t] = 1;
    }
    const long long p = p_lo + (long long)blockIdx.x;
    if (p >= p_hi) return;
    // p -> (i, j): plp_pair_index.hpp (two lists in one table, cross_n1 > 0: cell i of the first with cell j of the second)
    long long i, j;
    const bool known = pair_cells<LISTED>(p, true, n, cross_n1, list, i, j);
    if constexpr (LISTED) {
        if (!known) {  // (the whole wavefront: one pair per workgroup)
            if (lane == 0) compact[p - p_lo] = PAIR_BAD;
            return;
        }
    }
    const int mi = mrows ? mrows[i] : m_max;
    const int mj = mrows ? mrows[j] : m_max;
    const int m = mi + mj;
    const bool has = lane < m;
    const long long row = has ? ((lane < mi) ? i * m_max + lane : j * m_max + (lane - mi)) : 0;
    typename RowVec<NC>::type Tv;
    double T16;
    ChebyRow c;
    cheby_setup<D>(Tv, T16, c, lane, has, [&](int k) { return A[row * D + k]; },
                   [&]() { return b[row] + inflate; }, sh);  // b1 += abs_tol; b2 += abs_tol
    __syncthreads();
    const int st = cheby_run<D>(Tv, T16, c, lane, m, sh, m > 64);
    const double r = cheby_radius<D>(c);
    const bool yes = (st == ST_OPT) & (r > thresh);
    // (mark: "unbounded" / the iteration limit is not a verdict -- the careful pass that follows decides, plp_kernels.hpp)
    const unsigned char verdict = yes ? 1 : ((mark != 0) & ((st == ST_UNBND) | (st == ST_ITER)) ? PAIR_OPEN : 0);
    if (lane == 0) {
        if (compact) {
            compact[p - p_lo] = verdict;
        } else {
            adj[i * n + j] = verdict;
            adj[j * n + i] = verdict;
        }
    }
}

template <int D>
__global__ __launch_bounds__(64) void adjacent_w_kernel(int n, int m_max, const double* __restrict__ A,
                                                        const double* __restrict__ b, const int* __restrict__ mrows,
                                                        double inflate, double thresh, unsigned char* __restrict__ adj,
                                                        long long p_lo, long long p_hi, unsigned char* __restrict__ compact,
                                                        int cross_n1, int mark) {
    adjacent_w_body<D, false>(n, m_max, A, b, mrows, inflate, thresh, adj, p_lo, p_hi, compact, cross_n1, mark, nullptr);
}

// the listed pairs list[K][2] into out[K] (plp_pair_list): the same wavefront LP and verdict bytes
template <int D>
__global__ __launch_bounds__(64) void adjacent_w_list_kernel(int n, int m_max, const double* __restrict__ A,
                                                             const double* __restrict__ b, const int* __restrict__ mrows,
                                                             double inflate, double thresh, long long K,
                                                             const int* __restrict__ list, unsigned char* __restrict__ out,
                                                             int mark) {
    adjacent_w_body<D, true>(n, m_max, A, b, mrows, inflate, thresh, nullptr, 0, K, out, 0, mark, list);
}

// one pair per wavefront, d = 5..16: L.grid covers the pairs and, in the matrix form, the diagonal
int launch_adjacent_w(int d, const LpLaunch& L, const PairArgs& a, hipStream_t st) {
    return for_dim<5, MAX_D>(d, [&](auto K) {
        hipLaunchKernelGGL((adjacent_w_kernel<decltype(K)::value>), dim3((unsigned)L.grid), dim3(L.block), L.lds, st, a.n, a.m_max,
                           a.A, a.b, a.mrows, a.inflate, a.thresh, a.adj, a.p_lo, a.p_hi, a.compact, a.cross_n1, a.mark);
    });
}

// the listed form (a.list, a.p_hi pairs into a.compact)
int launch_adjacent_w_list(int d, const LpLaunch& L, const PairArgs& a, hipStream_t st) {
    return for_dim<5, MAX_D>(d, [&](auto K) {
        hipLaunchKernelGGL((adjacent_w_list_kernel<decltype(K)::value>), dim3((unsigned)L.grid), dim3(L.block), L.lds, st, a.n,
                           a.m_max, a.A, a.b, a.mrows, a.inflate, a.thresh, a.p_hi, a.list, a.compact, a.mark);
    });
}

// one LP per wavefront, d = 5..16
int launch_cheby_w(int d, const LpLaunch& L, const ChebyArgs& a, hipStream_t st) {
    return for_dim<5, MAX_D>(d, [&](auto K) {
        hipLaunchKernelGGL((cheby_w_kernel<decltype(K)::value>), dim3((unsigned)L.grid), dim3(L.block), L.lds, st, a.B, a.m_max, a.A,
                           a.b, a.mrows, a.r, a.xc, a.status);
    });
}

}  // namespace plp
