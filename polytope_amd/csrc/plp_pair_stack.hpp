// plp_pair_stack.hpp -- the stack of two cells of a packed table: what Polytope(np.vstack([A_i, A_j]), np.hstack([b_i,
// b_j])) holds (reference: Polytope.intersect, polytope/polytope.py:272-275; the constructor's row scaling, :130-138).
//
// For pair t = (i, j) of the table A[n][m_max][d], b[n][m_max], m[n] the stack has W = 2 m_max row slots:
//     slot s < m_i             row s of cell i
//     m_i <= s < m_i + m_j     row s - m_i of cell j
//     beyond                   no row
// Every row gets ONE constructor pass, fm::scale<D> (plp_fm.hpp: norm = sqrt of numpy's add.reduce of the squares,
// s = 1 / norm, a * s and b * s); a row of norm <= 1e-10 is dropped and the rows behind it move up.  ms[t] is the number of
// rows that stay; row slots from ms[t] on are zero.  m[p] is read clamped to 0..m_max, as the step kernels read it
// (plp_fm.hip); nothing at or beyond row m[p] of a cell is read.
//
// Which two cells pair t stacks is pair_cells<true> of plp_pair_index.hpp, with its validity rule: an index outside [0, n)
// or i == j is a bad pair, for which nothing of the table is read (ms = 0, every row zero).
//
// The same source compiles for the device (plp_pair_stack.hip) and for the host (tests/cabi/pair_stack_host.cpp, plain
// g++ -ffp-contract=off); host_stacks is the sequential restatement the device kernel is held against, bit for bit.
#pragma once
#include "plp_fm.hpp"
#include "plp_pair_index.hpp"

namespace plp {
namespace ps {

constexpr int MAX_W = 64;   // row slots of a stack (= MAX_M of the fused reduce that takes it)
constexpr int MAX_D = 16;

// rows cell p has in the table
PLP_FM_FN int cell_rows(const int* m, long long p, int m_max) {
    const int mp = m ? m[p] : m_max;
    return mp < 0 ? 0 : (mp > m_max ? m_max : mp);
}

// row slot s of the stack of cells (i, j) with mi / mj rows: the table row it comes from, or -1 (no row)
PLP_FM_FN long long source_row(long long i, long long j, int mi, int mj, int m_max, int s) {
    if (s < mi) return i * m_max + s;
    if (s < mi + mj) return j * m_max + (s - mi);
    return -1;
}

// table row `row` after its constructor pass -> x[D], bb; false: dropped
template <int D>
PLP_FM_FN bool stack_row(const double* A, const double* b, long long row, double* x, double& bb) {
    const double* a = A + (size_t)row * D;
#pragma unroll
    for (int c = 0; c < D; ++c) x[c] = a[c];
    bb = b[row];
    return fm::scale<D>(x, bb);
}

// ---- host side (plain functions: host-only under hipcc as well)
// the first bad pair of the list, or -1
static inline long long host_first_bad(int n, long long K, const int* pairs) {
    for (long long t = 0; t < K; ++t) {
        long long i, j;
        if (!pair_cells<true>(t, true, n, 0, pairs, i, j)) return t;
    }
    return -1;
}

// the sequential restatement: A_s[K][2 m_max][D], b_s[K][2 m_max], m_s[K]; a bad pair gets ms = 0 and zero rows
template <int D>
static inline void host_stacks_t(int n, int m_max, const double* A, const double* b, const int* m, long long K,
                                 const int* pairs, double* A_s, double* b_s, int* m_s) {
    const int W = 2 * m_max;
    for (long long t = 0; t < K; ++t) {
        long long i, j;
        const bool ok = pair_cells<true>(t, true, n, 0, pairs, i, j);
        const int mi = ok ? cell_rows(m, i, m_max) : 0, mj = ok ? cell_rows(m, j, m_max) : 0;
        double* Ao = A_s + (size_t)t * W * D;
        double* bo = b_s + (size_t)t * W;
        int out = 0;
        for (int s = 0; s < mi + mj; ++s) {
            double x[D], bb;
            if (!stack_row<D>(A, b, source_row(i, j, mi, mj, m_max, s), x, bb)) continue;
            for (int c = 0; c < D; ++c) Ao[(size_t)out * D + c] = x[c];
            bo[out++] = bb;
        }
        m_s[t] = out;
        for (int s = out; s < W; ++s) {
            for (int c = 0; c < D; ++c) Ao[(size_t)s * D + c] = 0.0;
            bo[s] = 0.0;
        }
    }
}

// 0, or 2: sizes outside 2 m_max <= 64, 1 <= d <= 16
static inline int host_stacks(int n, int m_max, int d, const double* A, const double* b, const int* m, long long K,
                              const int* pairs, double* A_s, double* b_s, int* m_s) {
    if (m_max < 1 || 2 * m_max > MAX_W) return 2;
#define PLP_PS_D(DD) \
    case DD: host_stacks_t<DD>(n, m_max, A, b, m, K, pairs, A_s, b_s, m_s); return 0;
    switch (d) {
        PLP_PS_D(1) PLP_PS_D(2) PLP_PS_D(3) PLP_PS_D(4) PLP_PS_D(5) PLP_PS_D(6) PLP_PS_D(7) PLP_PS_D(8) PLP_PS_D(9)
        PLP_PS_D(10) PLP_PS_D(11) PLP_PS_D(12) PLP_PS_D(13) PLP_PS_D(14) PLP_PS_D(15) PLP_PS_D(16)
        default: return 2;
    }
#undef PLP_PS_D
}

}  // namespace ps
}  // namespace plp
