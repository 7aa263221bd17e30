// What the host builds of the shared-row kernels (support_host.cpp, nearest_host.cpp) share: TEST INFRASTRUCTURE.
// run(): the batch in a plain sequential loop -- polytope by polytope, item by item, the rows of ONE polytope staged
// contiguously (LS = 1), no tile, no lanes, no rounds: nothing of the device's indexing (plp_row_tile.hpp) is emulated, which
// is what the bit-for-bit GPU tests rest on.  What one staged row is and what one item does are the caller's, the per-row
// and per-problem functions of the kernels.  Then the D x RV dispatch, and for the stand-alone programs (-D..._HOST_MAIN) a
// generator and the polytopes they make themselves.
#pragma once
#include <math.h>
#include <stdint.h>

#include <vector>

#include "../../polytope_amd/csrc/plp_row_tile.hpp"

namespace rowhost {

// ROW(p, a, b_i, live, n, s): row i of polytope p (a: its D entries, or those of row 0 when not live; b_i zero then -- rows
// i >= m[p] are not read) -> n[D], s[NS].  ITEM(p, j, q, m, cols, planes): item j of polytope p, q = p * K + j; cols[RV * D]
// and planes[NS][RV] its staged rows.
template <int D, int RV, int NS, class RowF, class ItemF>
void run(long long B, int m_max, const double* A, const double* b, const int* m, int K, RowF ROW, ItemF ITEM) {
    for (long long p = 0; p < B; ++p) {
        const int mk = plp::rowtile::clamp_rows(m ? m[p] : m_max, m_max);
        double cols[RV * D], planes[NS][RV];
        for (int i = 0; i < RV; ++i) {
            const bool live = i < mk;
            double n[D], s[NS];
            ROW(p, A + ((size_t)p * m_max + (live ? i : 0)) * D, live ? b[(size_t)p * m_max + i] : 0.0, live, n, s);
            for (int k = 0; k < D; ++k) cols[i * D + k] = n[k];
            for (int t = 0; t < NS; ++t) planes[t][i] = s[t];
        }
        for (int j = 0; j < K; ++j) ITEM(p, j, (size_t)p * K + j, mk, cols, planes);
    }
}

// f(dim<D>{}, rows<RV>{}) for the instance the launchers pick -> 0; 2 for a size the kernels do not take
template <class F>
int dispatch(int m_max, int d, int K, F&& f) {
    const int rv = plp::rowtile::row_slots(m_max);
    if (rv == 0 || K < 1) return 2;
    return plp::rowtile::dispatch(d, rv, f);
}

// xorshift64*, [0, 1)
struct Rng {
    uint64_t s = 0x9e3779b97f4a7c15ull;
    double unif() {
        s ^= s >> 12; s ^= s << 25; s ^= s >> 27;
        return (double)((s * 0x2545f4914f6cdd1dull) >> 11) * (1.0 / 9007199254740992.0);
    }
};

// (m_max, d) of the polytopes the programs make: every d and row-slot count, m_max = 0, fewer rows than a box has
constexpr int SHAPES[][2] = {{5, 1}, {7, 2}, {16, 3}, {17, 3}, {33, 4}, {64, 4}, {0, 2}, {3, 3}};
constexpr long long B_MADE = 23;

// B_MADE polytopes of m_max rows in R^d with ragged m: box rows |x_k| <= 3 first (bounded once m covers them), then
// b_i = CUT(p, a_i) for a_i uniform in [-1, 1)^d, which CUT may rescale
template <class CutF>
void make_polytopes(Rng& g, int m_max, int d, std::vector<double>& A, std::vector<double>& b, std::vector<int>& m, CutF CUT) {
    A.assign((size_t)B_MADE * m_max * d, 0.0);
    b.assign((size_t)B_MADE * m_max, 0.0);
    m.assign(B_MADE, 0);
    for (long long p = 0; p < B_MADE; ++p) {
        m[p] = m_max ? 1 + (int)(g.unif() * m_max) : 0;
        if (p % 5 == 0) m[p] = m_max;
        for (int i = 0; i < m_max; ++i) {
            double* a = &A[((size_t)p * m_max + i) * d];
            if (i < 2 * d) {
                a[i % d] = i < d ? 1.0 : -1.0;
                b[(size_t)p * m_max + i] = 3.0;
            } else {
                for (int k = 0; k < d; ++k) a[k] = 2.0 * g.unif() - 1.0;
                b[(size_t)p * m_max + i] = CUT(p, a);
            }
        }
    }
}

}  // namespace rowhost
