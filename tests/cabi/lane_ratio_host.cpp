// Host build of the ratio-test row loop of polytope_amd/csrc/plp_lane_lp.hpp (lane::ratio_rows: the one loop behind every
// tile shape of reduce_lane_kernel and bbox_lane_kernel) against a plain restatement of the formulas it replaced, written
// here: separate dot products, a subtraction for the slack, running selects, absolute row numbers.  TEST INFRASTRUCTURE,
// compiled with g++ -O2 -ffp-contract=off by tests/test_lane_ratio_host.py; with -DLANE_RATIO_MAIN it is a stand-alone
// program (the sanitizer build).  Everything is compared bit for bit, except the slack of the walk's pass (agree_walk).
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "../../polytope_amd/csrc/plp_lane_lp.hpp"

namespace {
using namespace plp::lane;

struct Rng {   // splitmix64
    uint64_t s;
    uint64_t next() {
        uint64_t z = (s += 0x9e3779b97f4a7c15ull);
        z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
        z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
        return z ^ (z >> 31);
    }
    double uni() { return (double)(next() >> 11) * (1.0 / 9007199254740992.0); }   // [0, 1)
    double sym() { return 2.0 * uni() - 1.0; }
    int below(int n) { return (int)(next() % (uint64_t)n); }
};

struct Best {
    double bs, bd;
    int bi;
};
bool same(const Best& p, const Best& q) { return memcmp(&p.bs, &q.bs, 8) == 0 && memcmp(&p.bd, &q.bd, 8) == 0 && p.bi == q.bi; }

// ---- the restatement: row-major A[rows][D], beta[rows]; rows i0 .. i0 + cnt - 1; krv < 0: nothing relaxed
double ref_dot(int D, const double* a, const double* v) {
    double s = a[0] * v[0];
    for (int k = 1; k < D; ++k) s = fma(a[k], v[k], s);
    return s;
}
// (d <= 3 is embedded in R^3: absent columns are zeros of a three-term chain, as in the kernel)
double ref_dot_embedded(int D, const double* a, const double* v) {
    if (D == 4) return ref_dot(4, a, v);
    double a3[3] = {a[0], D > 1 ? a[1] : 0.0, D > 2 ? a[2] : 0.0};
    return ref_dot(3, a3, v);
}
void ref_scan(int D, const double* A, const double* beta, int i0, int cnt, int krv, const double* d, const double* x, bool first,
              double tolp, Best& B) {
    for (int i = i0; i < i0 + cnt; ++i) {
        double bt = beta[i];
        if (i == krv) bt = bt + 0.1;
        const double ad = ref_dot_embedded(D, A + i * D, d);
        double sl;
        if (first) sl = fmax(bt, 0.0);
        else {
            const double ax = ref_dot_embedded(D, A + i * D, x);
            sl = fmax(bt - ax, 0.0);
        }
        const bool better = (ad > tolp) & (sl * B.bd < B.bs * ad);
        B.bs = better ? sl : B.bs;
        B.bd = better ? ad : B.bd;
        B.bi = better ? i : B.bi;
    }
}
// what the lanes of a pair / quad do with their candidates (plp_reduce_lane.hpp, `meet`): the smaller ratio, on ties the lower row
void ref_meet(Best& mine, const Best& other) {
    const double l = other.bs * mine.bd, r = mine.bs * other.bd;
    const bool theirs = (other.bd > 0.0) & (!(mine.bd > 0.0) | (l < r) | ((l == r) & (other.bi < mine.bi)));
    if (theirs) mine = other;
}

struct Stats {
    long long sets, mismatches, ties, none, relaxed, shares, axis, first, near_ties;
};

// The walk's pass forms the slack in ONE fma chain, the restatement with a dot product and a subtraction: the same row and
// the same a.d bit for bit, the slack within 1e-15 (|beta| + sum |a_j x_j|).  Another row only where the two best ratios lie
// within 4 ulp of each other (counted in near_ties).
bool near_ratio(const Best& p, const Best& q) {
    if (p.bi < 0 || q.bi < 0) return false;
    const double rp = p.bs / p.bd, rq = q.bs / q.bd;
    return fabs(rp - rq) <= 4 * 2.220446049250313e-16 * fmax(rp, rq);
}
bool agree_walk(int D, const Best& R, const Best& G, const double* A, const double* beta, int krv, const double* x, Stats& st) {
    if (R.bi != G.bi) {
        if (!near_ratio(R, G)) return false;
        st.near_ties++;
        return true;
    }
    if (R.bi < 0) return same(R, G);
    double mag = fabs(R.bi == krv ? beta[R.bi] + 0.1 : beta[R.bi]);
    for (int k = 0; k < D; ++k) mag += fabs(A[R.bi * D + k] * x[k]);
    return memcmp(&R.bd, &G.bd, 8) == 0 && fabs(R.bs - G.bs) <= 1e-15 * mag;
}

template <int D, int LS>
void run(long long n, uint64_t seed, Stats& st) {
    Rng g{seed * 1315423911ull + (uint64_t)D};
    static double tA[32 * D * LS], tb[32 * LS];   // the strided tile (slot p of LS), and the same rows row-major
    double A[32 * D], beta[32];
    for (long long t = 0; t < n; ++t) {
        const int rows = (t & 1) ? 32 : 16;
        const int p = g.below(LS);
        for (int i = 0; i < 32 * D * LS; ++i) tA[i] = g.sym();   // (other slots: other polytopes' rows, never read)
        for (int i = 0; i < 32 * LS; ++i) tb[i] = g.uni();
        for (int i = 0; i < rows; ++i) {
            for (int k = 0; k < D; ++k) A[i * D + k] = g.sym();
            beta[i] = g.uni() < 0.1 ? 0.0 : 2.0 * g.uni();
            if (g.uni() < 0.08) {   // a dead row, zeroed
                for (int k = 0; k < D; ++k) A[i * D + k] = 0.0;
                beta[i] = 0.0;
            }
        }
        const int kind = g.below(8);
        if (kind == 0) {   // duplicated rows: the lower one must win a tie
            for (int q = 0; q < 6; ++q) {
                const int a = g.below(rows), b = g.below(rows);
                for (int k = 0; k < D; ++k) A[b * D + k] = A[a * D + k];
                beta[b] = beta[a];
            }
        }
        for (int i = 0; i < rows; ++i) {
            for (int k = 0; k < D; ++k) tA[(i * D + k) * LS + p] = A[i * D + k];
            tb[i * LS + p] = beta[i];
        }
        double dv[4] = {0, 0, 0, 0}, xv[4] = {0, 0, 0, 0};
        for (int k = 0; k < (D < 3 ? 3 : D); ++k) { dv[k] = g.sym(); xv[k] = 0.3 * g.sym(); }   // (d < 3, embedded: the rest meet zero columns)
        double tolp = 1e-11 * (fabs(dv[0]) + fabs(dv[1]) + fabs(dv[2]) + fabs(dv[3]));
        if (kind == 1) tolp = 1e3;   // no eligible row
        const double (&dr)[4] = dv;
        const double (&xr)[4] = xv;
        // ---- the walk's pass, one share
        Best R{1.0, 0.0, -1}, G{1.0, 0.0, -1};
        ref_scan(D, A, beta, 0, rows, -1, dv, xv, false, tolp, R);
        ratio_rows<D, LS, RATIO_WALK, false>(tA + p, tb + p, 0, rows, -1, dr, xr, 0, 0.0, tolp, G.bs, G.bd, G.bi);
        st.sets++;
        if (!agree_walk(D, R, G, A, beta, -1, xv, st)) st.mismatches++;
        if (R.bi < 0) {
            st.none++;
            if (!(G.bi == -1 && G.bs == 1.0 && G.bd == 0.0)) st.mismatches++;
        }
        if (kind == 0 && G.bi >= 0) {
            for (int i = 0; i < rows; ++i)
                if (i != G.bi && memcmp(A + i * D, A + G.bi * D, 8 * D) == 0 && beta[i] == beta[G.bi]) {
                    st.ties++;
                    if (i < G.bi) st.mismatches++;   // a copy below the winner: the tie went the wrong way
                }
        }
        // ---- 2 and 4 shares, met by the lanes' rule, against the single scan
        for (int nparts = 2; nparts <= 4; nparts *= 2) {
            const int cnt = rows / nparts;
            Best part[4], rpart[4];
            for (int q = 0; q < nparts; ++q) {
                part[q] = Best{1.0, 0.0, -1};
                rpart[q] = Best{1.0, 0.0, -1};
                ratio_rows<D, LS, RATIO_WALK, false>(tA + p, tb + p, q * cnt, cnt, -1, dr, xr, 0, 0.0, tolp, part[q].bs, part[q].bd, part[q].bi);
                ref_scan(D, A, beta, q * cnt, cnt, -1, dv, xv, false, tolp, rpart[q]);
                if (!agree_walk(D, rpart[q], part[q], A, beta, -1, xv, st)) st.mismatches++;
            }
            // lane 0's view: xor 1, then xor 2 (whose partner has met its own neighbour)
            Best l0 = part[0], l2 = nparts > 2 ? part[2] : Best{1.0, 0.0, -1};
            ref_meet(l0, part[1]);
            if (nparts > 2) { ref_meet(l2, part[3]); ref_meet(l0, l2); }
            st.shares++;
            // the single scan's winner has the smallest ratio and, among equals, the lowest row: so has the met candidate.
            // Two rows whose ratios agree to rounding (d = 1: every row with beta = 0 is the same constraint, scaled) have no
            // order the cross-multiplied compare would keep across a different sequence of comparisons: counted, not failed,
            // when the two ratios lie within 4 ulp of each other.
            if (!same(l0, G)) {
                if (near_ratio(l0, G)) st.near_ties++;
                else st.mismatches++;
            }
        }
        // ---- the relaxed form (every k on one set in four, a random k otherwise), walk and first pass
        if constexpr (D >= 3) {
            const bool every = (t & 3) == 0;
            const int k0 = every ? 0 : g.below(rows), k1 = every ? rows : k0 + 1;
            for (int k = k0; k < k1; ++k) {
                for (int nparts = 1; nparts <= 4; nparts *= 2) {
                    const int cnt = rows / nparts, q = g.below(nparts);
                    Best r2{1.0, 0.0, -1}, g2{1.0, 0.0, -1};
                    ref_scan(D, A, beta, q * cnt, cnt, k, dv, xv, false, tolp, r2);
                    ratio_rows<D, LS, RATIO_WALK, true>(tA + p, tb + p, q * cnt, cnt, k, dr, xr, 0, 0.0, tolp, g2.bs, g2.bd, g2.bi);
                    st.relaxed++;
                    if (!agree_walk(D, r2, g2, A, beta, k, xv, st)) st.mismatches++;
                    if constexpr (D == 3) {
                        Best r3{1.0, 0.0, -1}, g3{1.0, 0.0, -1};
                        ref_scan(D, A, beta, q * cnt, cnt, k, dv, xv, true, tolp, r3);
                        ratio_rows<D, LS, RATIO_FIRST, true>(tA + p, tb + p, q * cnt, cnt, k, dr, xr, 0, 0.0, tolp, g3.bs, g3.bd, g3.bi);
                        if (!same(r3, g3)) st.mismatches++;
                    }
                }
            }
        }
        // ---- first passes (d <= 3): from x' = 0 the slack is beta -- the walk's formulas at x' = 0 find the same; and along
        // -+e_k one column is the whole a.d
        if constexpr (D <= 3) {
            const double zero[4] = {0, 0, 0, 0};
            Best r0{1.0, 0.0, -1}, rw{1.0, 0.0, -1}, g0{1.0, 0.0, -1};
            ref_scan(D, A, beta, 0, rows, -1, dv, zero, true, tolp, r0);
            ref_scan(D, A, beta, 0, rows, -1, dv, zero, false, tolp, rw);
            ratio_rows<D, LS, RATIO_FIRST, false>(tA + p, tb + p, 0, rows, -1, dr, zero, 0, 0.0, tolp, g0.bs, g0.bd, g0.bi);
            Best gw{1.0, 0.0, -1};   // the walk's pass AT x' = 0: its chain gives back beta exactly
            ratio_rows<D, LS, RATIO_WALK, false>(tA + p, tb + p, 0, rows, -1, dr, zero, 0, 0.0, tolp, gw.bs, gw.bd, gw.bi);
            st.first++;
            if (!same(r0, g0) || !same(r0, rw) || !same(g0, gw)) st.mismatches++;
            for (int it = 0; it < 2 * D; ++it) {
                const int kx = it >> 1;
                const double cs = (it & 1) ? -1.0 : 1.0;
                const double c[3] = {kx == 0 ? cs : 0.0, kx == 1 ? cs : 0.0, kx == 2 ? cs : 0.0};
                const double da[4] = {-c[0], -c[1], -c[2], 0.0};   // (walk3: d = -c, with its signed zeros)
                const double tol = 1e-11;
                const int nparts = 1 << g.below(3), cnt = rows / nparts, q = g.below(nparts);
                Best ra{1.0, 0.0, -1}, ga{1.0, 0.0, -1};
                ref_scan(D, A, beta, q * cnt, cnt, -1, da, zero, true, tol, ra);
                ratio_rows<D, LS, RATIO_AXIS, false>(tA + p, tb + p, q * cnt, cnt, -1, da, zero, kx, -cs, tol, ga.bs, ga.bd, ga.bi);
                st.axis++;
                if (!same(ra, ga)) st.mismatches++;
            }
        }
    }
}
}  // namespace

// stats[9]: sets, mismatches, ties seen, sets with no eligible row, relaxed scans, share combinations, axis passes, first passes,
// choices between two ratios within 4 ulp of each other (share combinations; the one-chain slack against the subtraction)
extern "C" int lane_ratio_check(long long n, unsigned long long seed, long long* stats) {
    Stats st;
    memset(&st, 0, sizeof st);
    run<3, 16>(n, seed, st);
    run<4, 8>(n, seed + 1, st);
    run<3, 1>(n / 8, seed + 2, st);
    run<2, 4>(n / 8, seed + 3, st);
    run<1, 4>(n / 8, seed + 4, st);
    memcpy(stats, &st, sizeof st);
    return st.mismatches == 0 ? 0 : 1;
}

#ifdef LANE_RATIO_MAIN
int main(int argc, char** argv) {
    long long stats[9];
    const int rc = lane_ratio_check(argc > 1 ? atoll(argv[1]) : 4000, 7, stats);
    printf("sets %lld mismatches %lld ties %lld none %lld relaxed %lld shares %lld axis %lld first %lld near_ties %lld\n", stats[0],
           stats[1], stats[2], stats[3], stats[4], stats[5], stats[6], stats[7], stats[8]);
    return rc;
}
#endif
