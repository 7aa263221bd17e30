// Host build of polytope_amd/csrc/plp_projhull.hpp (the rule of projhull_kernel: which LPs the iterative hull asks, in
// which order, and what their answers make of the point and facet lists): TEST INFRASTRUCTURE, compiled with g++
// -ffp-contract=off by tests/projhull_host.py.  Every LP the rule asks goes to a C callback, so the caller decides what the
// answer of an LP is and sees exactly which LPs are asked, in order; the enumeration of the facets is the sequential twin
// of the kernel's (projhull::enumerate).
//
// -DPROJHULL_HOST_MAIN adds a main(): a stand-alone program with an LP of its own for two polytopes whose support function
// is known in closed form (a cube, and a simplex given by its vertices), for a run under -fsanitize=address,undefined
// without anything loaded into an interpreter.
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <vector>

#include "../../polytope_amd/csrc/plp_projhull.hpp"

namespace ph = plp::projhull;

// max c . x over polytope p (c[d]: zero outside the kept coordinates) -> *lp_status (0 optimal, 3 unbounded, else failed)
// and x[d], a point of the polytope that attains it.  Returns 0, or a positive code that ends the call
typedef int (*ph_lp_fn)(long long p, int d, const double* c, int* lp_status, double* x, void* user);

namespace {

template <int K>
int one(const long long p, const int m_max, const int d, const double* A, const double* b, int m, const int* keep,
        const double* xc, const int f_max, const int max_lps, ph_lp_fn fn, void* user, double* Ao, double* bo, uint64_t* on,
        int32_t* count, double* V, int32_t* nv, double* X, uint64_t* vmask, int32_t* nlp, int32_t* status, int32_t* nrank) {
    static ph::State<K> S;   // (13 KiB: not on the stack of a callback-driven call)
    m = m < 0 ? 0 : (m > m_max ? m_max : m);
    // the rows as the kernel stages them: beta_i = b_i - a_i . xc, the sum as an fma chain in column order
    std::vector<double> beta(m);
    bool nocentre = m < 1;
    double babs = 0.0;
    for (int i = 0; i < m; ++i) {
        double s = 0.0;
        bool finite = true;
        for (int t = 0; t < d; ++t) {
            const double v = A[(size_t)i * d + t];
            s = t == 0 ? v * xc[t] : fma(v, xc[t], s);
            finite = finite && isfinite(v);
        }
        beta[i] = b[i] - s;
        if (!(finite && beta[i] > 0.0 && isfinite(beta[i]))) nocentre = true;
        babs = fmax(babs, fabs(beta[i]));
    }
    ph::begin(S, d, keep, f_max, max_lps, babs);
    int rc = 0;
    if (nocentre) ph::done(S, ph::PH_NOCENTRE);
    while (!nocentre) {
        const int req = ph::step(S, X);
        if (req == ph::REQ_DONE) break;
        if (req == ph::REQ_ENUM) {
            ph::enumerate(S);
            continue;
        }
        std::vector<double> c(d, 0.0), x(d, 0.0);
        for (int j = 0; j < K; ++j) c[keep[j]] = S.dir[j];
        int st = -1;
        rc = fn(p, d, c.data(), &st, x.data(), user);
        if (rc) break;
        S.lp_status = st;
        double viol = -__builtin_inf();
        bool isnan_any = false;
        for (int i = 0; i < m && st == ph::LP_OPT; ++i) {
            double r = 0.0;
            for (int t = 0; t < d; ++t) r = r + A[(size_t)i * d + t] * (x[t] - xc[t]);
            const double v = r - beta[i];
            isnan_any = isnan_any || v != v;
            viol = fmax(viol, v);
        }
        S.lp_viol = isnan_any ? __builtin_nan("") : viol;
        for (int t = 0; t < d; ++t) S.lp_x[t] = x[t];
    }
    if (rc) return rc;
    ph::finish_rows<K>(S, f_max, Ao, bo, on, 0, 1);
    ph::finish_points<K>(S, V, X, 0, 1);
    *count = ph::out_count(S);
    *nv = S.nv;
    *vmask = ph::vertex_mask<K>(S);
    *nlp = S.nlp;
    *status = S.status;
    *nrank = S.nrank;
    return 0;
}

}  // namespace

// All B polytopes, one after the other, as the kernel's wavefronts take them; the arrays of plp_project_hull_batch, and
// nrank[B]: the points the rank step added.  Returns 0, the callback's code, or -1 for sizes beyond the caps.
extern "C" int projhull_host(long long B, int m_max, int d, int k, const double* A, const double* b, const int32_t* m,
                             const int32_t* keep, const double* xc, int f_max, int max_lps, ph_lp_fn fn, void* user, double* Ao,
                             double* bo, uint64_t* on, int32_t* count, double* V, int32_t* nv, double* X, uint64_t* vmask,
                             int32_t* nlp, int32_t* status, int32_t* nrank) {
    if (k < 1 || k > ph::MAX_K || d < k || d > ph::MAX_D || m_max < 0 || m_max > ph::MAX_ROWS || f_max < 1 || f_max > ph::F_CAP)
        return -1;
    for (int t = 0; t < k; ++t)
        if (keep[t] < 0 || keep[t] >= d || (t && keep[t] <= keep[t - 1])) return -1;
    for (long long p = 0; p < B; ++p) {
        const double* Ap = A + (size_t)p * m_max * d;
        const double* bp = b + (size_t)p * m_max;
        const int mp = m ? m[p] : m_max;
        double* Xp = X ? X + (size_t)p * ph::MAX_POINTS * d : nullptr;
        int rc;
#define PH_ONE(KK)                                                                                                           \
    rc = one<KK>(p, m_max, d, Ap, bp, mp, keep, xc + (size_t)p * d, f_max, max_lps, fn, user, Ao + (size_t)p * f_max * KK,    \
                 bo + (size_t)p * f_max, on + (size_t)p * f_max, count + p, V + (size_t)p * ph::MAX_POINTS * KK, nv + p, Xp, \
                 vmask + p, nlp + p, status + p, nrank + p)
        if (k == 1) PH_ONE(1);
        else if (k == 2) PH_ONE(2);
        else PH_ONE(3);
#undef PH_ONE
        if (rc) return rc;
    }
    return 0;
}

#ifdef PROJHULL_HOST_MAIN
#include <stdio.h>

namespace {

// a polytope as the hull of its vertices: the LP is a maximum over them (ties: the first)
struct Verts {
    int d, n;
    const double* P;
    long long asked;
};
int verts_lp(long long, int d, const double* c, int* lp_status, double* x, void* user) {
    Verts& T = *static_cast<Verts*>(user);
    T.asked++;
    int best = 0;
    double bv = -__builtin_inf();
    for (int i = 0; i < T.n; ++i) {
        double v = 0.0;
        for (int t = 0; t < d; ++t) v += c[t] * T.P[i * d + t];
        if (v > bv) {
            bv = v;
            best = i;
        }
    }
    for (int t = 0; t < d; ++t) x[t] = T.P[best * d + t];
    *lp_status = 0;
    return 0;
}

// runs one polytope given by rows AND vertices; the facets to expect: `want` rows; buffers of exactly the declared sizes
int run_case(const char* name, int m, int d, int k, const double* A, const double* b, const int32_t* keep, const double* xc,
             int nvert, const double* P, int want_status, int want_count, int max_lps, int f_max) {
    Verts T{d, nvert, P, 0};
    std::vector<double> Ao((size_t)f_max * k), bo(f_max), V((size_t)ph::MAX_POINTS * k), X((size_t)ph::MAX_POINTS * d);
    std::vector<uint64_t> on(f_max);
    uint64_t vmask = 0;
    int32_t count = -1, nv = -1, nlp = -1, status = -1, nrank = -1;
    const int rc = projhull_host(1, m, d, k, A, b, nullptr, keep, xc, f_max, max_lps, verts_lp, &T, Ao.data(), bo.data(), on.data(),
                                 &count, V.data(), &nv, X.data(), &vmask, &nlp, &status, &nrank);
    bool ok = rc == 0 && status == want_status && count == want_count && nlp == (int)T.asked && nlp <= max_lps;
    // every vertex satisfies every row; every row is reached by a vertex
    for (int f = 0; ok && f < count; ++f) {
        double top = -__builtin_inf();
        for (int i = 0; i < nvert; ++i) {
            double v = 0.0;
            for (int j = 0; j < k; ++j) v += Ao[(size_t)f * k + j] * P[i * d + keep[j]];
            top = fmax(top, v);
        }
        ok = fabs(top - bo[f]) <= 1e-7;
    }
    printf("projhull_host: %-14s status %d count %d nv %d nlp %d nrank %d vmask %llx %s\n", name, status, count, nv, nlp, nrank,
           (unsigned long long)vmask, ok ? "ok" : "INCONSISTENT");
    return ok ? 0 : 1;
}

}  // namespace

int main() {
    int bad = 0;
    // the cube [-1, 1]^4 shifted, onto 1, 2 and 3 coordinates
    {
        const int d = 4;
        double A[8 * 4] = {0}, b[8], P[16 * 4], xc[4] = {0.5, -0.25, 2.0, 0.0};
        for (int t = 0; t < d; ++t) {
            A[(2 * t) * d + t] = 1.0;
            A[(2 * t + 1) * d + t] = -1.0;
            b[2 * t] = 1.0 + xc[t];
            b[2 * t + 1] = 1.0 - xc[t];
        }
        for (int i = 0; i < 16; ++i)
            for (int t = 0; t < d; ++t) P[i * d + t] = xc[t] + (((i >> t) & 1) ? 1.0 : -1.0);
        const int32_t k1[1] = {2}, k2[2] = {0, 3}, k3[3] = {0, 1, 3};
        bad += run_case("cube 4 -> 1", 8, d, 1, A, b, k1, xc, 16, P, ph::PH_OK, 2, 1000, 2);
        bad += run_case("cube 4 -> 2", 8, d, 2, A, b, k2, xc, 16, P, ph::PH_OK, 4, 1000, 64);
        bad += run_case("cube 4 -> 3", 8, d, 3, A, b, k3, xc, 16, P, ph::PH_OK, 6, 1000, 124);
        bad += run_case("cube budget", 8, d, 2, A, b, k2, xc, 16, P, ph::PH_BUDGET, 0, 3, 64);
        bad += run_case("cube f_max", 8, d, 2, A, b, k2, xc, 16, P, ph::PH_OVERFLOW_FACETS, 0, 1000, 2);
    }
    // a simplex in R^3 onto 2 coordinates, and the triangle whose box points are collinear, lifted to R^4
    {
        const int d = 3;
        const double P[4 * 3] = {0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 1};
        const double s3 = 1.0 / sqrt(3.0);
        const double A[4 * 3] = {-1, 0, 0, 0, -1, 0, 0, 0, -1, s3, s3, s3}, b[4] = {0, 0, 0, s3}, xc[3] = {0.2, 0.2, 0.2};
        const int32_t k2[2] = {0, 2};
        bad += run_case("simplex 3 -> 2", 4, d, 2, A, b, k2, xc, 4, P, ph::PH_OK, 3, 1000, 64);
    }
    {
        const int d = 4;
        const double P[3 * 4] = {0, 0, 0, 0, 1, 1, 0, 0, 0.5, 0.2, 0, 0};
        // (the rows are not read by this LP; a centre with positive slack to rows that hold it)
        const double A[2 * 4] = {1, 0, 0, 0, -1, 0, 0, 0}, b[2] = {2, 1}, xc[4] = {0.5, 0.4, 0, 0};
        const int32_t k2[2] = {0, 1};
        bad += run_case("collinear start", 2, d, 2, A, b, k2, xc, 3, P, ph::PH_OK, 3, 1000, 64);
    }
    printf("projhull_host: inconsistent: %d\n", bad);
    return bad ? 1 : 0;
}
#endif
