// Host build of walk3 (polytope_amd/csrc/plp_lane_lp.hpp) in BOTH forms: TEST INFRASTRUCTURE, compiled with g++ by
// tests/test_lane_walk_ab_host.py.  This file is compiled twice -- with -DPLP_LANE_PLAIN_WALK (the one general loop) and
// without (peeled second and third pass, rows fetched together) -- and the two objects are linked into one
// library: lane_walk_run_plain / lane_walk_run_peeled run every box (F3) and redundancy (F2) LP of a packed batch and
// return the final Lp3 of each, field by field, with a tally of the walk's exits and passes (PLP_LANE_TALLY).
// With -DLANE_WALK_AB_MAIN the peeled object carries a main() that makes its own batches (centre at the origin), runs both
// forms and compares them: the stand-alone program for sanitizer runs.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

namespace {
long long g_tally[32];
}
#define PLP_LANE_TALLY(e) (++g_tally[(e)])
#include "../../polytope_amd/csrc/plp_lane_lp.hpp"

#ifdef PLP_LANE_PLAIN_WALK
#define LANE_WALK_RUN lane_walk_run_plain
#else
#define LANE_WALK_RUN lane_walk_run_peeled
#endif

// A[B][16][3] (columns >= dim zero, rows >= mrows[p] zero), beta[B][16] = max(b - A xc, 0), relax[B][16] = max((b + 0.1) - A xc, 0).
// LPs of polytope p, in this order: the 2 dim box LPs (lower_0, upper_0, ...), then the redundancy LP of every row k < mrows[p]
// (cost -a_k, row k's right-hand side relax[k]).  xs[n][3]: x0..x2; is[n][7]: w0, w1, w2, nact, status, iters, ndeg;
// tally[WE_COUNT] is ADDED to.  Returns the number of LPs (xs / is may be null: count only).
extern "C" long long LANE_WALK_RUN(long long B, int dim, const double* A, const double* beta, const double* relax,
                                   const int* mrows, double* xs, int* is, long long* tally) {
    memset(g_tally, 0, sizeof g_tally);
    long long n = 0;
    for (long long p = 0; p < B; ++p) {
        const double* Ap = A + p * 48;
        const int m = mrows[p];
        auto one = [&](const double* c, const double* bt) {
            if (xs) {
                plp::lane::Lp3 S;
                plp::lane::solve3<16>(
                    S, c[0], c[1], c[2], true,
                    [&](int i, double& a0, double& a1, double& a2) { a0 = Ap[i * 3]; a1 = Ap[i * 3 + 1]; a2 = Ap[i * 3 + 2]; },
                    [&](int i) { return bt[i]; }, [](bool q) { return q; });
                xs[n * 3] = S.x0; xs[n * 3 + 1] = S.x1; xs[n * 3 + 2] = S.x2;
                int* o = is + n * 7;
                o[0] = S.w0; o[1] = S.w1; o[2] = S.w2; o[3] = S.nact; o[4] = S.status; o[5] = S.iters; o[6] = S.ndeg;
            }
            ++n;
        };
        for (int it = 0; it < 2 * dim; ++it) {
            double c[3] = {0, 0, 0};
            c[it >> 1] = (it & 1) ? -1.0 : 1.0;
            one(c, beta + p * 16);
        }
        for (int k = 0; k < m; ++k) {
            const double c[3] = {-Ap[k * 3], -Ap[k * 3 + 1], -Ap[k * 3 + 2]};
            double bt[16];
            memcpy(bt, beta + p * 16, sizeof bt);
            bt[k] = relax[p * 16 + k];
            one(c, bt);
        }
    }
    if (tally)
        for (int e = 0; e < plp::lane::WE_COUNT; ++e) tally[e] += g_tally[e];
    return n;
}

#if defined(LANE_WALK_AB_MAIN) && !defined(PLP_LANE_PLAIN_WALK)
#include <vector>

extern "C" long long lane_walk_run_plain(long long B, int dim, const double* A, const double* beta, const double* relax,
                                         const int* mrows, double* xs, int* is, long long* tally);

namespace {
uint64_t g_rng = 0x9e3779b97f4a7c15ull;
double uni() {   // (0, 1)
    g_rng = g_rng * 6364136223846793005ull + 1442695040888963407ull;
    return ((double)(g_rng >> 11) + 0.5) * (1.0 / 9007199254740992.0);
}
double nrm() {   // roughly normal: a sum of uniforms
    double s = 0.0;
    for (int i = 0; i < 6; ++i) s += uni();
    return (s - 3.0) * 1.4142135623730951;
}
}  // namespace

int main() {
    const int B = 600;
    long long bad = 0, total = 0;
    long long tp[32] = {0}, tq[32] = {0};
    for (int dim = 1; dim <= 3; ++dim) {
        for (int fam = 0; fam < 4; ++fam) {   // random, box with cuts, open prism, rows a hair apart
            std::vector<double> A(B * 48, 0.0), beta(B * 16, 0.0), relax(B * 16, 0.0);
            std::vector<int> mrows(B, 0);
            for (int p = 0; p < B; ++p) {
                int m = fam == 0 ? 1 + (int)(uni() * 16) : (fam == 1 ? 2 * dim + (int)(uni() * 5) : 4 + (int)(uni() * 12));
                double* Ap = &A[p * 48];
                for (int i = 0; i < m; ++i) {
                    double v[3] = {0, 0, 0}, l = 0.0;
                    for (int k = 0; k < dim; ++k) { v[k] = nrm(); l += v[k] * v[k]; }
                    if (fam == 2 && dim >= 2) { l -= v[dim - 1] * v[dim - 1]; v[dim - 1] = 0.0; }   // open along the last axis
                    l = sqrt(l);
                    if (!(l > 1e-3)) { v[0] = 1.0; l = 1.0; }
                    for (int k = 0; k < 3; ++k) Ap[i * 3 + k] = v[k] / l;
                    beta[p * 16 + i] = 0.5 + uni();
                }
                if (fam == 1)
                    for (int i = 0; i < 2 * dim; ++i) {
                        for (int k = 0; k < 3; ++k) Ap[i * 3 + k] = (k == (i >> 1)) ? ((i & 1) ? -1.0 : 1.0) : 0.0;
                        beta[p * 16 + i] = 0.5 * (1 + (int)(uni() * 3));
                    }
                if (fam == 3) {
                    const int i = (int)(uni() * m), j = (i + 1 + (int)(uni() * (m - 1))) % m;
                    const double eps = (p % 3 == 0) ? 0.0 : ((p % 3 == 1) ? 1e-9 : 1e-6);
                    for (int k = 0; k < dim; ++k) Ap[j * 3 + k] = Ap[i * 3 + k] + eps * nrm();
                    beta[p * 16 + j] = beta[p * 16 + i] + ((p & 1) ? 1e-7 : 0.0);
                }
                mrows[p] = m;
                for (int i = 0; i < m; ++i) relax[p * 16 + i] = beta[p * 16 + i] + 0.1;
            }
            const long long n = lane_walk_run_plain(B, dim, A.data(), beta.data(), relax.data(), mrows.data(), nullptr, nullptr, nullptr);
            std::vector<double> xp(n * 3), xq(n * 3);
            std::vector<int> ip(n * 7), iq(n * 7);
            lane_walk_run_plain(B, dim, A.data(), beta.data(), relax.data(), mrows.data(), xp.data(), ip.data(), tp);
            lane_walk_run_peeled(B, dim, A.data(), beta.data(), relax.data(), mrows.data(), xq.data(), iq.data(), tq);
            total += n;
            if (memcmp(xp.data(), xq.data(), sizeof(double) * 3 * n) != 0 || memcmp(ip.data(), iq.data(), sizeof(int) * 7 * n) != 0) {
                ++bad;
                printf("dim %d family %d: the two forms differ\n", dim, fam);
            }
        }
    }
    printf("%lld LPs, %lld batches differ\n", total, bad);
    printf("tally plain :");
    for (int e = 0; e < plp::lane::WE_COUNT; ++e) printf(" %lld", tp[e]);
    printf("\ntally peeled:");
    for (int e = 0; e < plp::lane::WE_COUNT; ++e) printf(" %lld", tq[e]);
    printf("\n");
    return bad ? 1 : 0;
}
#endif
