// Host build of polytope_amd/csrc/plp_support.hpp (the per-LP function of support_kernel, plp_support.hip): TEST
// INFRASTRUCTURE, compiled with g++ -ffp-contract=off by tests/support_host.py.  support_host is plp_support_batch in the
// plain loop of row_tile_host.hpp: per polytope the rows staged as the kernel stages them (a_i, beta_i = b_i - a_i.xc, zero
// rows beyond m), then one solve_one per direction -- the device's answers are held against these bit for bit.
//
// -DSUPPORT_HOST_MAIN adds a main(): a stand-alone program that runs the same loop on polytopes it makes itself (boxes
// with random cuts, ragged m, every d and row-slot count, interior / boundary / NaN centres), for a run under
// -fsanitize=address,undefined without anything loaded into an interpreter.
#include "../../polytope_amd/csrc/plp_support.hpp"
#include "row_tile_host.hpp"

// the arguments of plp_support_batch without the context; 0, or 2 for a size the kernel does not take
extern "C" int support_host(long long B, int m_max, int d, const double* A, const double* b, const int* m, int K,
                            const double* C, int c_shared, const double* xc, double* val, double* x, int* status) {
    return rowhost::dispatch(m_max, d, K, [&](auto dim, auto rows) {
        constexpr int D = decltype(dim)::value, RV = decltype(rows)::value;
        rowhost::run<D, RV, 1>(
            B, m_max, A, b, m, K,
            [&](long long p, const double* a, double bi, bool live, auto& n, auto& s) {
                for (int k = 0; k < D; ++k) n[k] = live ? a[k] : 0.0;
                s[0] = live ? plp::support::beta_of<D>(a, bi, xc + p * D) : 0.0;
            },
            [&](long long p, int j, size_t lp, int mk, const double* sA, const auto& planes) {
                const double* csrc = C + (c_shared ? (size_t)j : lp) * D;
                double c[4] = {0.0, 0.0, 0.0, 0.0}, xcp[4] = {0.0, 0.0, 0.0, 0.0}, xo[4], v;
                for (int k = 0; k < D; ++k) {
                    c[k] = csrc[k];
                    xcp[k] = xc[p * D + k];
                }
                int st;
                plp::support::solve_one<D, RV>(sA, planes[0], 1, mk, c, xcp, true, [](bool q) { return q; }, v, xo, st);
                val[lp] = v;
                status[lp] = st;
                if (x)
                    for (int k = 0; k < D; ++k) x[lp * D + k] = xo[k];
            });
    });
}

// polytopes per workgroup the launcher picks for (K, m_max): the tests cross it with their batch sizes
extern "C" int support_polytopes_per_group(int K, int m_max) {
    const int rv = plp::rowtile::row_slots(m_max);
    return rv ? plp::rowtile::polytopes_per_group(K, rv) : 0;
}

#ifdef SUPPORT_HOST_MAIN
#include <stdio.h>

int main() {
    long long lps = 0, n0 = 0, n1 = 0, n3 = 0, bad = 0;
    rowhost::Rng g;
    for (const auto& sh : rowhost::SHAPES) {
        const int m_max = sh[0], d = sh[1];
        for (int K : {1, 3, 9, 65}) {
            for (int c_shared = 0; c_shared < 2; ++c_shared) {
                const long long B = rowhost::B_MADE;
                std::vector<double> A, b, xc((size_t)B * d);
                std::vector<double> C((c_shared ? (size_t)K : (size_t)B * K) * d), val((size_t)B * K), x((size_t)B * K * d);
                std::vector<int> m, st((size_t)B * K);
                rowhost::make_polytopes(g, m_max, d, A, b, m, [&](long long, double* a) {   // unit cuts at 1 .. 2
                    double nn = 0.0;
                    for (int k = 0; k < d; ++k) nn += a[k] * a[k];
                    for (int k = 0; k < d; ++k) a[k] /= sqrt(nn) + 1e-300;
                    return 1.0 + g.unif();
                });
                for (long long p = 0; p < B; ++p) {
                    // centres: near the origin (inside), on the first box facet, NaN
                    for (int k = 0; k < d; ++k) xc[(size_t)p * d + k] = 0.2 * (g.unif() - 0.5);
                    if (p % 7 == 3) xc[(size_t)p * d] = 3.0;
                    if (p % 11 == 5) xc[(size_t)p * d + d - 1] = __builtin_nan("");
                }
                for (double& v : C) v = 2.0 * g.unif() - 1.0;
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
