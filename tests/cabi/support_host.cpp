// Host build of polytope_amd/csrc/plp_support.hpp (the per-LP function of support_kernel, plp_support.hip): TEST
// INFRASTRUCTURE, compiled with g++ -ffp-contract=off by tests/support_host.py.  support_host is plp_support_batch in a
// plain loop: per polytope the rows staged as the kernel stages them (a_i, beta_i = b_i - a_i.xc, zero rows beyond m),
// then one solve_one per direction -- the device's answers are held against these bit for bit.
//
// -DSUPPORT_HOST_MAIN adds a main(): a stand-alone program that runs the same loop on polytopes it makes itself (boxes
// with random cuts, ragged m, every d and row-slot count, interior / boundary / NaN centres), for a run under
// -fsanitize=address,undefined without anything loaded into an interpreter.
#include <stdint.h>

#include "../../polytope_amd/csrc/plp_support.hpp"

namespace {

template <int D, int RV>
void run_d(long long B, int m_max, const double* A, const double* b, const int* m, int K, const double* C, int c_shared,
           const double* xc, double* val, double* x, int* status) {
    for (long long p = 0; p < B; ++p) {
        int mk = m ? m[p] : m_max;
        mk = mk < 0 ? 0 : (mk > m_max ? m_max : mk);
        double sA[RV * D], sbeta[RV], xcp[4] = {0.0, 0.0, 0.0, 0.0};
        for (int k = 0; k < D; ++k) xcp[k] = xc[p * D + k];
        for (int i = 0; i < RV; ++i) {
            const bool live = i < mk;
            const double* src = A + ((size_t)p * m_max + (live ? i : 0)) * D;
            for (int k = 0; k < D; ++k) sA[i * D + k] = live ? src[k] : 0.0;
            sbeta[i] = live ? plp::support::beta_of<D>(src, b[(size_t)p * m_max + i], xcp) : 0.0;
        }
        for (int j = 0; j < K; ++j) {
            const size_t lp = (size_t)p * K + j;
            const double* csrc = C + (c_shared ? (size_t)j : lp) * D;
            double c[4] = {0.0, 0.0, 0.0, 0.0}, xo[4], v;
            for (int k = 0; k < D; ++k) c[k] = csrc[k];
            int st;
            plp::support::solve_one<D, RV>(sA, sbeta, 1, mk, c, xcp, true, [](bool q) { return q; }, v, xo, st);
            val[lp] = v;
            status[lp] = st;
            if (x)
                for (int k = 0; k < D; ++k) x[lp * D + k] = xo[k];
        }
    }
}

template <int D>
void run_rv(long long B, int m_max, const double* A, const double* b, const int* m, int K, const double* C, int c_shared,
            const double* xc, double* val, double* x, int* status) {
    const int rv = plp::support::row_slots(m_max);
    if (rv == 16) run_d<D, 16>(B, m_max, A, b, m, K, C, c_shared, xc, val, x, status);
    else if (rv == 32) run_d<D, 32>(B, m_max, A, b, m, K, C, c_shared, xc, val, x, status);
    else run_d<D, 64>(B, m_max, A, b, m, K, C, c_shared, xc, val, x, status);
}

}  // namespace

// the arguments of plp_support_batch without the context; 0, or 2 for a size the kernel does not take
extern "C" int support_host(long long B, int m_max, int d, const double* A, const double* b, const int* m, int K,
                            const double* C, int c_shared, const double* xc, double* val, double* x, int* status) {
    if (d < 1 || d > 4 || plp::support::row_slots(m_max) == 0 || K < 1) return 2;
    switch (d) {
        case 1: run_rv<1>(B, m_max, A, b, m, K, C, c_shared, xc, val, x, status); break;
        case 2: run_rv<2>(B, m_max, A, b, m, K, C, c_shared, xc, val, x, status); break;
        case 3: run_rv<3>(B, m_max, A, b, m, K, C, c_shared, xc, val, x, status); break;
        default: run_rv<4>(B, m_max, A, b, m, K, C, c_shared, xc, val, x, status); break;
    }
    return 0;
}

// polytopes per workgroup the launcher picks for (K, m_max): the tests cross it with their batch sizes
extern "C" int support_polytopes_per_group(int K, int m_max) {
    const int rv = plp::support::row_slots(m_max);
    return rv ? plp::support::polytopes_per_group(K, rv) : 0;
}

#ifdef SUPPORT_HOST_MAIN
#include <stdio.h>

#include <vector>

namespace {
uint64_t g_s = 0x9e3779b97f4a7c15ull;
double unif() {   // xorshift64*, [0, 1)
    g_s ^= g_s >> 12; g_s ^= g_s << 25; g_s ^= g_s >> 27;
    return (double)((g_s * 0x2545f4914f6cdd1dull) >> 11) * (1.0 / 9007199254740992.0);
}
}  // namespace

int main() {
    long long lps = 0, n0 = 0, n1 = 0, n3 = 0, bad = 0;
    const int shapes[][2] = {{5, 1}, {7, 2}, {16, 3}, {17, 3}, {33, 4}, {64, 4}, {0, 2}, {3, 3}};
    for (const auto& sh : shapes) {
        const int m_max = sh[0], d = sh[1];
        for (int K : {1, 3, 9, 65}) {
            for (int c_shared = 0; c_shared < 2; ++c_shared) {
                const long long B = 23;
                std::vector<double> A((size_t)B * m_max * d), b((size_t)B * m_max), xc((size_t)B * d);
                std::vector<double> C((c_shared ? (size_t)K : (size_t)B * K) * d), val((size_t)B * K), x((size_t)B * K * d);
                std::vector<int> m(B), st((size_t)B * K);
                for (long long p = 0; p < B; ++p) {
                    m[p] = m_max ? 1 + (int)(unif() * m_max) : 0;
                    if (p % 5 == 0) m[p] = m_max;
                    for (int i = 0; i < m_max; ++i) {
                        double* a = &A[((size_t)p * m_max + i) * d];
                        if (i < 2 * d) {   // box rows |x_k| <= 3 first: bounded once m covers them
                            for (int k = 0; k < d; ++k) a[k] = 0.0;
                            a[i % d] = i < d ? 1.0 : -1.0;
                            b[(size_t)p * m_max + i] = 3.0;
                        } else {
                            double nn = 0.0;
                            for (int k = 0; k < d; ++k) { a[k] = 2.0 * unif() - 1.0; nn += a[k] * a[k]; }
                            for (int k = 0; k < d; ++k) a[k] /= sqrt(nn) + 1e-300;
                            b[(size_t)p * m_max + i] = 1.0 + unif();
                        }
                    }
                    // centres: near the origin (inside), on the first box facet, NaN
                    for (int k = 0; k < d; ++k) xc[(size_t)p * d + k] = 0.2 * (unif() - 0.5);
                    if (p % 7 == 3) xc[(size_t)p * d] = 3.0;
                    if (p % 11 == 5) xc[(size_t)p * d + d - 1] = __builtin_nan("");
                }
                for (double& v : C) v = 2.0 * unif() - 1.0;
                for (int k = 0; k < d && K > 1; ++k) C[k] = 0.0;   // a zero direction
                for (int with_x = 0; with_x < 2; ++with_x) {
                    if (support_host(B, m_max, d, A.data(), b.data(), m.data(), K, C.data(), c_shared, xc.data(), val.data(),
                                     with_x ? x.data() : nullptr, st.data()) != 0) { ++bad; continue; }
                    for (size_t q = 0; q < st.size(); ++q) {
                        ++lps;
                        n0 += st[q] == 0; n1 += st[q] == 1; n3 += st[q] == 3;
                        bad += !(st[q] == 0 || st[q] == 1 || st[q] == 3) || (st[q] == 0 && !isfinite(val[q]));
                    }
                }
            }
        }
    }
    printf("support_host: %lld LPs, status 0: %lld, 1: %lld, 3: %lld, inconsistent: %lld\n", lps, n0, n1, n3, bad);
    return bad ? 1 : 0;
}
#endif
