// Host build of polytope_amd/csrc/plp_pair_dist.hpp (the per-pair function of pair_dist_kernel, plp_pair_dist.hip): TEST
// INFRASTRUCTURE, compiled with g++ -ffp-contract=off by tests/pair_dist_host.py.  pair_dist_host is plp_pair_dist in a plain
// loop: per listed pair the rows of the two cells staged as the kernel stages them (a_i, beta_i = b_i - a_i.xc, zero rows
// beyond m; LS = 1, no tile, no lanes), then one solve_pair that works both cells -- the device, which puts the two cells
// of a pair on two lanes, is held against these answers bit for bit.
//
// -DPAIR_DIST_HOST_MAIN adds a main(): a stand-alone program for a run under -fsanitize=address,undefined without anything
// loaded into an interpreter.  It runs the same loop over the records of the files named on its command line (written by
// tests/pair_dist_host.py: write_records -- int64 n, m_max, d, K, then A, b, xc as doubles, m and pairs as int32), or,
// without arguments, over cells it makes itself.
#include "../../polytope_amd/csrc/plp_pair_dist.hpp"
#include "row_tile_host.hpp"

// the arguments of plp_pair_dist without the context (rounds[K] or NULL: support rounds per pair); 0, 2 for a size the kernel
// does not take, 1 for a pair that is not two different cells of [0, n) -- nothing is written then
extern "C" int pair_dist_host(int n, int m_max, int d, const double* A, const double* b, const int* m, const double* xc,
                              long long K, const int* pairs, double* dist, double* lb, double* x, double* y, int* status,
                              int* rounds) {
    for (long long t = 0; t < K; ++t) {
        const int i = pairs[2 * t], j = pairs[2 * t + 1];
        if (i < 0 || i >= n || j < 0 || j >= n || i == j) return 1;
    }
    return rowhost::dispatch(m_max, d, 1, [&](auto dim, auto rows) {
        constexpr int D = decltype(dim)::value, RV = decltype(rows)::value;
        for (long long t = 0; t < K; ++t) {
            double cols[2][RV * D], beta[2][RV], c[2][4] = {{0.0, 0.0, 0.0, 0.0}, {0.0, 0.0, 0.0, 0.0}};
            int mk[2];
            for (int s = 0; s < 2; ++s) {
                const long long p = pairs[2 * t + s];
                mk[s] = plp::rowtile::clamp_rows(m ? m[p] : m_max, m_max);
                for (int k = 0; k < D; ++k) c[s][k] = xc[p * D + k];
                for (int i = 0; i < RV; ++i) {
                    const bool live = i < mk[s];
                    const double* a = A + ((size_t)p * m_max + (live ? i : 0)) * D;
                    double av[D], cv[D];
                    for (int k = 0; k < D; ++k) {
                        av[k] = live ? a[k] : 0.0;
                        cv[k] = live ? c[s][k] : 0.0;
                        cols[s][i * D + k] = av[k];
                    }
                    beta[s][i] = live ? plp::support::beta_of<D>(av, b[(size_t)p * m_max + i], cv) : 0.0;
                }
            }
            double dd, l, xo[D], yo[D];
            int st, rd;
            plp::pairdist::solve_pair<D, RV>(cols[0], beta[0], mk[0], c[0], cols[1], beta[1], mk[1], c[1], 1, dd, l, xo, yo, st, rd);
            dist[t] = dd;
            status[t] = st;
            if (lb) lb[t] = l;
            if (rounds) rounds[t] = rd;
            for (int k = 0; k < D; ++k) {
                if (x) x[t * D + k] = xo[k];
                if (y) y[t * D + k] = yo[k];
            }
        }
    });
}

extern "C" int pair_dist_max_rounds() { return plp::pairdist::MAX_ROUNDS; }
// pairs per workgroup at m_max rows: the tests cross it with their list lengths
extern "C" int pair_dist_pairs_per_group(int m_max) {
    const int rv = plp::rowtile::row_slots(m_max);
    return rv ? plp::rowtile::polytopes_per_group(1, rv) / 2 : 0;
}

#ifdef PAIR_DIST_HOST_MAIN
#include <stdio.h>

namespace {
long long g_n = 0, g_c[4] = {0, 0, 0, 0}, g_bad = 0;

void run_record(int n, int m_max, int d, long long K, const double* A, const double* b, const int* m, const double* xc,
                const int* pairs) {
    std::vector<double> dist(K), lb(K), x((size_t)K * d), y((size_t)K * d);
    std::vector<int> st(K), rd(K);
    for (int full = 0; full < 2; ++full) {
        if (pair_dist_host(n, m_max, d, A, b, m, xc, K, pairs, dist.data(), full ? lb.data() : nullptr, full ? x.data() : nullptr,
                           full ? y.data() : nullptr, st.data(), full ? rd.data() : nullptr) != 0) { ++g_bad; return; }
        for (long long q = 0; q < K; ++q) {
            ++g_n;
            const bool known = st[q] == 0 || st[q] == 1 || st[q] == 3;
            if (known) ++g_c[st[q]];
            g_bad += !known || (st[q] == 0 && !(dist[q] >= 0.0)) || (st[q] != 0 && dist[q] == dist[q]);
        }
    }
}
}  // namespace

int main(int argc, char** argv) {
    for (int f = 1; f < argc; ++f) {
        FILE* fp = fopen(argv[f], "rb");
        if (!fp) { fprintf(stderr, "pair_dist_host: cannot open %s\n", argv[f]); return 2; }
        int64_t hd[4];
        while (fread(hd, sizeof(int64_t), 4, fp) == 4) {
            const int n = (int)hd[0], m_max = (int)hd[1], d = (int)hd[2];
            const long long K = hd[3];
            std::vector<double> A((size_t)n * m_max * d), b((size_t)n * m_max), xc((size_t)n * d);
            std::vector<int> m(n), pairs((size_t)K * 2);
            if (fread(A.data(), 8, A.size(), fp) != A.size() || fread(b.data(), 8, b.size(), fp) != b.size() ||
                fread(xc.data(), 8, xc.size(), fp) != xc.size() || fread(m.data(), 4, m.size(), fp) != m.size() ||
                fread(pairs.data(), 4, pairs.size(), fp) != pairs.size()) {
                fprintf(stderr, "pair_dist_host: short record in %s\n", argv[f]);
                fclose(fp);
                return 2;
            }
            run_record(n, m_max, d, K, A.data(), b.data(), m.data(), xc.data(), pairs.data());
        }
        fclose(fp);
    }
    if (argc < 2) {
        rowhost::Rng g;
        for (const auto& sh : rowhost::SHAPES) {
            const int m_max = sh[0], d = sh[1], n = (int)rowhost::B_MADE;
            std::vector<double> A, b, xc((size_t)n * d, 0.0);
            std::vector<int> m, pairs;
            rowhost::make_polytopes(g, m_max, d, A, b, m, [&](long long, double*) { return 1.0 + g.unif(); });   // (the origin is inside)
            for (int p = 0; p < n; ++p) {   // cell p moved by t_p: b += A t, xc = t; one centre is not a number
                for (int k = 0; k < d; ++k) xc[(size_t)p * d + k] = 9.0 * g.unif() - 4.5;
                for (int i = 0; i < m_max; ++i)
                    for (int k = 0; k < d; ++k) b[(size_t)p * m_max + i] += A[((size_t)p * m_max + i) * d + k] * xc[(size_t)p * d + k];
            }
            xc[(size_t)5 * d] = __builtin_nan("");
            for (int t = 0; t < 60; ++t) {
                const int i = (int)(g.unif() * n), j = (int)(g.unif() * n);
                if (i != j) { pairs.push_back(i); pairs.push_back(j); }
            }
            run_record(n, m_max, d, (long long)pairs.size() / 2, A.data(), b.data(), m.data(), xc.data(), pairs.data());
        }
    }
    printf("pair_dist_host: %lld pairs, status 0: %lld, 1: %lld, 3: %lld, inconsistent: %lld\n", g_n, g_c[0], g_c[1], g_c[3], g_bad);
    return g_bad ? 1 : 0;
}
#endif
