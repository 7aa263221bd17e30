// Host build of walk3 (polytope_amd/csrc/plp_lane_lp.hpp) with and without the vertex round of its general loop: TEST
// INFRASTRUCTURE, compiled with g++ by tests/test_lane_state_ab_host.py.  This file is compiled twice -- with the default
// flags (the vertex round in the general loop) and with -DPLP_LANE_WIDE_STATE -DPLP_LANE_NO_VERTEX_ROUND (one kind of general
// pass; the header's walk state has one form, its seven integers in a field of Lp3 each, so the first flag only names the
// build) -- and the two objects are linked into one library: lane_state_run_packed (the default build) /
// lane_state_run_wide run every box (F3) and redundancy (F2) LP of a packed batch from the centre, then every box LP again
// WARM, from the point its predecessor ended on (a vertex, an edge or a facet point), and return the final Lp3 of each,
// field by field, with the tallies of the walk (PLP_LANE_TALLY).
// With -DLANE_STATE_AB_MAIN the default object carries a main() that makes its own batches (centre at the origin), runs
// both forms and compares them: the stand-alone program for sanitizer runs.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

namespace {
long long g_tally[32];
}
#define PLP_LANE_TALLY(e) (++g_tally[(e)])
#include "../../polytope_amd/csrc/plp_lane_lp.hpp"
static_assert(sizeof g_tally / sizeof g_tally[0] >= plp::lane::WE_COUNT_ALL, "a tally array holds WE_COUNT_ALL entries");

#ifdef PLP_LANE_WIDE_STATE
#define LANE_STATE_RUN lane_state_run_wide
#else
#define LANE_STATE_RUN lane_state_run_packed
#endif

// A[B][16][3] (columns >= dim zero, rows >= mrows[p] zero), beta[B][16] = max(b - A xc, 0), relax[B][16] = max((b + 0.1) - A xc, 0).
// LPs of polytope p, in this order: the 2 dim box LPs (lower_0, upper_0, ...) from the centre; the redundancy LP of every
// row k < mrows[p] (cost -a_k, row k's right-hand side relax[k]); then box LP (it + 1) mod 2 dim started warm from where
// box LP `it` ended, for every `it` that ended optimal on at least one row (iters = ndeg = 0, as walk3 asks).
// xs[n][3]: x0..x2; is[n][7]: w0, w1, w2, nact, status, iters, ndeg; tally[WE_COUNT_ALL] and warm_from[4] (warm starts by
// the nact they began with) are ADDED to.  Returns the number of LPs (xs / is may be null: count only).
extern "C" long long LANE_STATE_RUN(long long B, int dim, const double* A, const double* beta, const double* relax,
                                    const int* mrows, double* xs, int* is, long long* tally, long long* warm_from) {
    memset(g_tally, 0, sizeof g_tally);
    long long n = 0;
    for (long long p = 0; p < B; ++p) {
        const double* Ap = A + p * 48;
        const int m = mrows[p];
        auto one = [&](plp::lane::Lp3& S, const double* c, const double* bt, bool warm) {
            plp::lane::solve3<16>(
                S, c[0], c[1], c[2], true,
                [&](int i, double& a0, double& a1, double& a2) { a0 = Ap[i * 3]; a1 = Ap[i * 3 + 1]; a2 = Ap[i * 3 + 2]; },
                [&](int i) { return bt[i]; }, [](bool q) { return q; }, warm);
            if (xs) {
                xs[n * 3] = S.x0; xs[n * 3 + 1] = S.x1; xs[n * 3 + 2] = S.x2;
                int* o = is + n * 7;
                o[0] = S.w0; o[1] = S.w1; o[2] = S.w2; o[3] = S.nact; o[4] = S.status; o[5] = S.iters; o[6] = S.ndeg;
            }
            ++n;
        };
        auto box_cost = [](int it, double* c) {
            c[0] = c[1] = c[2] = 0.0;
            c[it >> 1] = (it & 1) ? -1.0 : 1.0;
        };
        plp::lane::Lp3 ends[6];
        for (int it = 0; it < 2 * dim; ++it) {
            double c[3];
            box_cost(it, c);
            one(ends[it], c, beta + p * 16, false);
        }
        for (int k = 0; k < m; ++k) {
            const double c[3] = {-Ap[k * 3], -Ap[k * 3 + 1], -Ap[k * 3 + 2]};
            double bt[16];
            memcpy(bt, beta + p * 16, sizeof bt);
            bt[k] = relax[p * 16 + k];
            plp::lane::Lp3 S;
            one(S, c, bt, false);
        }
        for (int it = 0; it < 2 * dim; ++it) {
            plp::lane::Lp3 S = ends[it];
            if (S.status != plp::ST_OPT || S.nact < 1) continue;
            if (warm_from) ++warm_from[S.nact];
            S.iters = 0;
            S.ndeg = 0;
            double c[3];
            box_cost((it + 1) % (2 * dim), c);
            one(S, c, beta + p * 16, true);
        }
    }
    if (tally)
        for (int e = 0; e < plp::lane::WE_COUNT_ALL; ++e) tally[e] += g_tally[e];
    return n;
}

#if defined(LANE_STATE_AB_MAIN) && !defined(PLP_LANE_WIDE_STATE)
#include <vector>

extern "C" long long lane_state_run_wide(long long B, int dim, const double* A, const double* beta, const double* relax,
                                         const int* mrows, double* xs, int* is, long long* tally, long long* warm_from);

namespace {
uint64_t g_rng = 0x2545f4914f6cdd1dull;
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
    const int B = 40;
    long long bad = 0, total = 0;
    long long tp[32] = {0}, tq[32] = {0}, wp[4] = {0}, wq[4] = {0};
    for (int dim = 1; dim <= 3; ++dim) {
        for (int fam = 0; fam < 4; ++fam) {   // random, box with cuts, open prism, rows a hair apart
            std::vector<double> A(B * 48, 0.0), beta(B * 16, 0.0), relax(B * 16, 0.0);
            std::vector<int> mrows(B, 0);
            for (int p = 0; p < B; ++p) {
                const int m = fam == 0 ? 1 + (int)(uni() * 16) : (fam == 1 ? 2 * dim + (int)(uni() * 5) : 4 + (int)(uni() * 12));
                double* Ap = &A[p * 48];
                for (int i = 0; i < m; ++i) {
                    double v[3] = {0, 0, 0}, l = 0.0;
                    for (int k = 0; k < dim; ++k) { v[k] = nrm(); l += v[k] * v[k]; }
                    if (fam == 2 && dim >= 2) { l -= v[dim - 1] * v[dim - 1]; v[dim - 1] = 0.0; }   // open along the last axis
                    l = sqrt(l);
                    if (!(l > 1e-3)) { v[0] = 1.0; v[1] = v[2] = 0.0; l = 1.0; }
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
            const long long cap = (long long)B * (4 * dim + 16);   // (no form can issue more: 2 dim cold, m <= 16, 2 dim warm)
            std::vector<double> xp(cap * 3), xq(cap * 3);
            std::vector<int> ip(cap * 7), iq(cap * 7);
            const long long n = lane_state_run_wide(B, dim, A.data(), beta.data(), relax.data(), mrows.data(), xp.data(), ip.data(), tp, wp);
            const long long nq = lane_state_run_packed(B, dim, A.data(), beta.data(), relax.data(), mrows.data(), xq.data(), iq.data(), tq, wq);
            total += n;
            if (nq != n || memcmp(xp.data(), xq.data(), sizeof(double) * 3 * n) != 0 || memcmp(ip.data(), iq.data(), sizeof(int) * 7 * n) != 0) {
                ++bad;
                printf("dim %d family %d: the two forms differ\n", dim, fam);
            }
        }
    }
    printf("%lld LPs, %lld batches differ\n", total, bad);
    printf("tally wide  :");
    for (int e = 0; e < plp::lane::WE_COUNT_ALL; ++e) printf(" %lld", tp[e]);
    printf("\ntally packed:");
    for (int e = 0; e < plp::lane::WE_COUNT_ALL; ++e) printf(" %lld", tq[e]);
    printf("\nwarm starts from a facet / an edge / a vertex: %lld / %lld / %lld\n", wq[1], wq[2], wq[3]);
    return bad ? 1 : 0;
}
#endif
