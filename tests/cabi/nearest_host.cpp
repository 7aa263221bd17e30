// Host build of polytope_amd/csrc/plp_nearest.hpp (the per-problem function of nearest_kernel, plp_nearest.hip): TEST
// INFRASTRUCTURE, compiled with g++ -ffp-contract=off by tests/nearest_host.py.  nearest_host is plp_nearest_batch in the
// plain loop of row_tile_host.hpp: per polytope the rows staged as the kernel stages them (n_i, beta_i, |a_i|, zero rows
// beyond m), then one solve_one per point -- the device's answers are held against these bit for bit.
//
// -DNEAREST_HOST_MAIN adds a main(): a stand-alone program for a run under -fsanitize=address,undefined without anything
// loaded into an interpreter.  It runs the same loop over the records of the files named on its command line (written by
// tests/nearest_host.py: write_records -- int64 B, m_max, d, K, x_shared, then A, b as doubles, m as int32, X as doubles),
// or, without arguments, over polytopes it makes itself.
#include "../../polytope_amd/csrc/plp_nearest.hpp"
#include "row_tile_host.hpp"

// the arguments of plp_nearest_batch without the context; 0, or 2 for a size the kernel does not take
extern "C" int nearest_host(long long B, int m_max, int d, const double* A, const double* b, const int* m, int K,
                            const double* X, int x_shared, double* dist, double* x, uint64_t* face, double* lam, int* status) {
    return rowhost::dispatch(m_max, d, K, [&](auto dim, auto rows) {
        constexpr int D = decltype(dim)::value, RV = decltype(rows)::value;
        rowhost::run<D, RV, 2>(
            B, m_max, A, b, m, K,
            [](long long, const double* a, double bi, bool live, auto& n, auto& s) {
                plp::nearest::stage_row<D>(a, bi, live, n, s[0], s[1]);
            },
            [&](long long, int j, size_t q, int mk, const double* sN, const auto& planes) {
                const double* src = X + (x_shared ? (size_t)j : q) * D;
                double pt[D], xo[D], lo[D], dd;
                for (int k = 0; k < D; ++k) pt[k] = src[k];
                uint64_t fc;
                int st;
                plp::nearest::solve_one<D, RV>(sN, planes[0], planes[1], 1, mk, pt, dd, xo, fc, lo, st);
                dist[q] = dd;
                status[q] = st;
                if (face) face[q] = fc;
                for (int k = 0; k < D; ++k) {
                    if (x) x[q * D + k] = xo[k];
                    if (lam) lam[q * D + k] = lo[k];
                }
            });
    });
}

// polytopes per workgroup and points of one K-chunk the launcher picks for (K, m_max): the tests cross them with their sizes
extern "C" int nearest_polytopes_per_group(int K, int m_max) {
    const int rv = plp::rowtile::row_slots(m_max);
    return rv ? plp::rowtile::polytopes_per_group(K, rv) : 0;
}
extern "C" int nearest_chunk_points(int K, int m_max) {
    const int rv = plp::rowtile::row_slots(m_max);
    if (!rv) return 0;
    const int L = 64 / plp::rowtile::polytopes_per_group(K, rv);
    return plp::nearest::chunk_rounds(K, L) * L;
}
extern "C" int nearest_iter_cap(int m, int d) { return plp::nearest::iter_cap(m, d); }

#ifdef NEAREST_HOST_MAIN
#include <stdio.h>

namespace {
long long g_n = 0, g_c[3] = {0, 0, 0}, g_bad = 0;

void run_record(long long B, int m_max, int d, int K, int x_shared, const double* A, const double* b, const int* m,
                const double* X) {
    const size_t n = (size_t)B * K;
    std::vector<double> dist(n), x(n * d), lam(n * d);
    std::vector<uint64_t> face(n);
    std::vector<int> st(n);
    for (int full = 0; full < 2; ++full) {
        if (nearest_host(B, m_max, d, A, b, m, K, X, x_shared, dist.data(), full ? x.data() : nullptr, full ? face.data() : nullptr,
                         full ? lam.data() : nullptr, st.data()) != 0) { ++g_bad; return; }
        for (size_t q = 0; q < n; ++q) {
            ++g_n;
            const bool known = st[q] == 0 || st[q] == 1 || st[q] == 2;
            if (known) ++g_c[st[q]];
            g_bad += !known || (st[q] == 0 && !(dist[q] >= 0.0)) || (st[q] != 0 && dist[q] == dist[q]);
        }
    }
}
}  // namespace

int main(int argc, char** argv) {
    for (int f = 1; f < argc; ++f) {
        FILE* fp = fopen(argv[f], "rb");
        if (!fp) { fprintf(stderr, "nearest_host: cannot open %s\n", argv[f]); return 2; }
        int64_t hd[5];
        while (fread(hd, sizeof(int64_t), 5, fp) == 5) {
            const long long B = hd[0];
            const int m_max = (int)hd[1], d = (int)hd[2], K = (int)hd[3], xs = (int)hd[4];
            std::vector<double> A((size_t)B * m_max * d), b((size_t)B * m_max), X((xs ? (size_t)K : (size_t)B * K) * d);
            std::vector<int> m(B);
            if (fread(A.data(), 8, A.size(), fp) != A.size() || fread(b.data(), 8, b.size(), fp) != b.size() ||
                fread(m.data(), 4, m.size(), fp) != m.size() || fread(X.data(), 8, X.size(), fp) != X.size()) {
                fprintf(stderr, "nearest_host: short record in %s\n", argv[f]);
                fclose(fp);
                return 2;
            }
            run_record(B, m_max, d, K, xs, A.data(), b.data(), m.data(), X.data());
        }
        fclose(fp);
    }
    if (argc < 2) {
        rowhost::Rng g;
        for (const auto& sh : rowhost::SHAPES) {
            const int m_max = sh[0], d = sh[1];
            for (int K : {1, 9, 65}) {
                for (int xs = 0; xs < 2; ++xs) {
                    const long long B = rowhost::B_MADE;
                    std::vector<double> A, b, X((xs ? (size_t)K : (size_t)B * K) * d);
                    std::vector<int> m;
                    rowhost::make_polytopes(g, m_max, d, A, b, m,   // (some are empty)
                                            [&](long long p, double*) { return p % 7 == 3 ? -4.0 : 1.0 + g.unif(); });
                    for (double& v : X) v = 12.0 * g.unif() - 6.0;
                    if (K > 1) X[0] = __builtin_nan("");
                    run_record(B, m_max, d, K, xs, A.data(), b.data(), m.data(), X.data());
                }
            }
        }
    }
    printf("nearest_host: %lld problems, status 0: %lld, 1: %lld, 2: %lld, inconsistent: %lld\n", g_n, g_c[0], g_c[1], g_c[2], g_bad);
    return g_bad ? 1 : 0;
}
#endif
