// plp_pair_index.hpp -- which two cells pair number p of a pair batch stacks: the one map of the engines' kernels
// (adjacent_r_kernel, plp_cheby_r_impl.hpp; adjacent_w_kernel, plp_wide.hip) and of the careful pass that follows them
// (careful_pairs_kernel, plp_verify.hip).
//
//   LISTED = false   p = i (i - 1) / 2 + j with j < i (all pairs of n cells, or a range of them); cross_n1 > 0: the table
//                    holds two lists, n1 cells then n - n1 cells, and p = a (n - n1) + c pairs cell a of the first with cell
//                    c of the second.
//   LISTED = true    the caller's list: pair p is (list[2 p], list[2 p + 1]) (plp_pair_list).  A pair with an index outside
//                    [0, n) or with i == j is not solved and nothing of the table is read for it: the map returns false,
//                    (i, j) = (0, 0), and the kernels write PAIR_BAD for it.
//
// The listed form is a template instantiation of its own, so the kernels of the dense calls keep their code.
//
// The same source compiles for the device and, for the host restatements of the tests (plp_pair_stack.hpp), under plain g++.
#pragma once
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define PLP_PAIR_FN __host__ __device__ __forceinline__
#else
#include <math.h>
#define PLP_PAIR_FN static inline
#endif

namespace plp {

constexpr unsigned char PAIR_BAD = 255;  // = PLP_PAIR_BAD (include/plp.h)

// `valid`: p is a pair of the launch (lanes beyond the batch get a harmless pair and read nothing)
template <bool LISTED>
PLP_PAIR_FN bool pair_cells(long long p, bool valid, int n, int cross_n1, const int* __restrict__ list, long long& i,
                            long long& j) {
    if constexpr (LISTED) {
        const int a = valid ? list[2 * p] : 0, c = valid ? list[2 * p + 1] : 0;
        const bool ok = valid & ((unsigned)a < (unsigned)n) & ((unsigned)c < (unsigned)n) & (a != c);
        i = ok ? a : 0;
        j = ok ? c : 0;
        return ok;
    } else {
        i = valid ? (long long)((1.0 + sqrt(1.0 + 8.0 * (double)p)) * 0.5) : 1;
        while (i * (i - 1) / 2 > p) --i;
        while ((i + 1) * i / 2 <= p) ++i;
        j = valid ? p - i * (i - 1) / 2 : 0;
        if (cross_n1 > 0) {
            const long long n2 = n - cross_n1;
            i = valid ? p / n2 : 0;
            j = valid ? cross_n1 + (p - i * n2) : 0;
        }
        return valid;
    }
}

}  // namespace plp
