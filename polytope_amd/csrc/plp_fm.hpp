// plp_fm.hpp -- the per-row arithmetic of one Fourier-Motzkin elimination step (reference: projection_fm,
// polytope/polytope.py:1911-1952) and of the Polytope constructor's row scaling (:130-138).
//
// One step takes the rows a previous reduce() kept, applies what the host would have done to them on the way (the
// (b + 0.1) - 0.1 round trip of a minimal representation, one constructor pass per Polytope built from them), splits them
// on column `col` into P (a > tol), Q (a < -tol) and N (|a| < tol) -- a coefficient of exactly +-tol is in none of the
// three and its row is dropped, as in the reference (:1925-1927) -- and forms, in the reference's order,
//     for j in P: for k in Q:  (-a_k,col) x_j + a_j,col x_k        then for j in N:  x_j
// with column `col` removed, each row scaled by the reciprocal of its norm (rows of norm <= 1e-10 dropped).
//
// The combination.  The reference forms the rows as np.dot(C, A) / np.dot(C, b) with two non-zero terms per row; which
// rounding that gets depends on the BLAS kernel that runs, so there is nothing stable to reproduce.  The engine fixes ONE
// formula, on the device and on the host alike (the build uses -ffp-contract=off, so nothing else is fused):
//     y = fma(a_j,col, x_k, (-a_k,col) * x_j)          (the P row's term rounded, the Q row's term fused)
// for every column of A and for b.  N rows are copied (1 * x_j is exact).
//
// The norm is sqrt of numpy's add.reduce of the squares over the row (pairwise: one running sum below 8 elements, eight
// running sums over blocks of eight beyond -- the same order as plp::np_dot in plp_common.hpp).
//
// The same source compiles for the device (plp_fm.hip) and for the host (tests/cabi/fm_host.cpp).
#pragma once
#include <math.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define PLP_FM_FN __host__ __device__ __forceinline__
#else
#define PLP_FM_FN static inline
#endif

namespace plp {
namespace fm {

constexpr double NORM_MIN = 1e-10;   // Polytope.__init__: rows with norm <= 1e-10 are dropped (ref :133)
constexpr double MINREP_SHIFT = 0.1; // reduce(): h[k] += 0.1; h[k] -= 0.1 (ref :1149-1151)

enum : int { CLS_N = 0, CLS_P = 1, CLS_Q = 2, CLS_NONE = 3 };

// P / Q / N split of one coefficient (ref :1925-1927)
PLP_FM_FN int classify(double a, double tol) {
    if (a > tol) return CLS_P;
    if (a < -tol) return CLS_Q;
    if (fabs(a) < tol) return CLS_N;
    return CLS_NONE;
}

// numpy's add.reduce(x * x) over a contiguous row of N doubles
template <int N>
PLP_FM_FN double sumsq(const double* x) {
    if constexpr (N < 8) {
        double s = 0.0;
#pragma unroll
        for (int k = 0; k < N; ++k) s = s + x[k] * x[k];
        return s;
    } else {
        double r[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) r[j] = x[j] * x[j];
        constexpr int BLK = N - N % 8;
#pragma unroll
        for (int i = 8; i < BLK; i += 8) {
#pragma unroll
            for (int j = 0; j < 8; ++j) r[j] = r[j] + x[i + j] * x[i + j];
        }
        double res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
#pragma unroll
        for (int i = BLK; i < N; ++i) res = res + x[i] * x[i];
        return res;
    }
}

// one pass of the constructor's scaling; false: the row is dropped
template <int N>
PLP_FM_FN bool scale(double* x, double& b) {
    const double nrm = sqrt(sumsq<N>(x));
    if (!(nrm > NORM_MIN)) return false;
    const double s = 1.0 / nrm;
#pragma unroll
    for (int k = 0; k < N; ++k) x[k] = x[k] * s;
    b = b * s;
    return true;
}

// what the host does to a row a previous step's reduce() kept before it reaches the next elimination:
// shift (minimal representation: (b + 0.1) - 0.1), then `passes` constructor passes; false: dropped on the way
template <int D>
PLP_FM_FN bool stage(double* x, double& b, bool shift, int passes) {
    if (shift) b = (b + MINREP_SHIFT) - MINREP_SHIFT;
    bool ok = true;
    for (int p = 0; p < passes; ++p) ok = ok && scale<D>(x, b);
    return ok;
}

// x[col] for a runtime col without a dynamic register index
template <int D>
PLP_FM_FN double pick(const double* x, int col) {
    double v = 0.0;
#pragma unroll
    for (int c = 0; c < D; ++c) v = (c == col) ? x[c] : v;
    return v;
}

// y[0..D-2] = x without column col
template <int D>
PLP_FM_FN void drop_col(const double* x, int col, double* y) {
#pragma unroll
    for (int c = 0; c + 1 < D; ++c) y[c] = (c < col) ? x[c] : x[c + 1];
}

// the combined row of P row j and Q row k, column col removed, scaled; false: dropped (norm <= 1e-10)
template <int D>
PLP_FM_FN bool combine(const double* xj, double bj, const double* xk, double bk, int col, double* y, double& yb) {
    const double aj = pick<D>(xj, col);
    const double nak = -pick<D>(xk, col);
    double full[D];
#pragma unroll
    for (int c = 0; c < D; ++c) full[c] = fma(aj, xk[c], nak * xj[c]);
    yb = fma(aj, bk, nak * bj);
    drop_col<D>(full, col, y);
    return scale<D - 1>(y, yb);
}

// an N row, column col removed, scaled; false: dropped
template <int D>
PLP_FM_FN bool pass_through(const double* xj, double bj, int col, double* y, double& yb) {
    drop_col<D>(xj, col, y);
    yb = bj;
    return scale<D - 1>(y, yb);
}

}  // namespace fm
}  // namespace plp
