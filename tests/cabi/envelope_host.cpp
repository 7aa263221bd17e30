// Host build of polytope_amd/csrc/plp_envelope.hpp (the rule of envelope_cross_kernel: which facets of which member are
// tested against which partner, in which order, and what the radii make of them): TEST INFRASTRUCTURE, compiled with g++
// -ffp-contract=off by tests/envelope_host.py.  Every radius the rule reads is asked from a C callback together with the
// stack it belongs to, so the caller decides what the radius of a stack is and sees exactly which stacks are asked, in order.
//
// -DENVELOPE_HOST_MAIN adds a main(): a stand-alone program that reads regions, the radius of every test their entries ask
// and the outputs to expect from a text file (written by the test from its own run) and runs the rule again, for a run
// under -fsanitize=address,undefined without anything loaded into an interpreter.
#include <stdint.h>
#include <string.h>

#include <vector>

#include "../../polytope_amd/csrc/plp_envelope.hpp"

namespace env = plp::env;

// the test of row ii of list entry w against the entry at list position j: stack[n][d + 1] = [rows of j; -row ii] -> *R.
// 0, or a positive code that ends the call
typedef int (*env_radius_fn)(long long w, long long j, int ii, int n, const double* stack, double* R, void* user);

namespace {

struct HostOracle {
    int d, mc_max;
    const double *A, *b;
    const int32_t *mc, *mem_idx;
    long long lo, w, own;   // the list starts at lo; this entry; its member
    env_radius_fn fn;
    void* user;
    long long j = 0, c = 0;
    int mj = 0, rc = 0;
    std::vector<double> stack;

    void partner(const long long jj) {
        j = jj;
        c = mem_idx ? (long long)mem_idx[lo + jj] : lo + jj;
        mj = env::member_rows(mc, mc_max, c);
        stack.assign((size_t)(mj + 1) * (d + 1), 0.0);
        for (int r = 0; r < mj; ++r) {
            for (int k = 0; k < d; ++k) stack[(size_t)r * (d + 1) + k] = A[(c * mc_max + r) * d + k];
            stack[(size_t)r * (d + 1) + d] = b[c * mc_max + r];
        }
    }
    double radius(const int ii) {
        for (int k = 0; k < d; ++k) stack[(size_t)mj * (d + 1) + k] = -A[(own * mc_max + ii) * d + k];
        stack[(size_t)mj * (d + 1) + d] = -b[own * mc_max + ii];
        double R = 0.0;
        if (!rc) rc = fn(w, j, ii, mj + 1, stack.data(), &R, user);
        return rc ? 0.0 : R;   // (after a failed callback the walk runs out on radii of 0: the call returns its code)
    }
};

}  // namespace

// All L list entries, one after the other, as the kernel's wavefronts take them.  Returns 0, the callback's code, or -1
// for a d beyond the cap.
extern "C" int envelope_host(int d, long long C, int mc_max, const double* A, const double* b, const int32_t* mc, long long B,
                             const int32_t* reg_off, long long L, const int32_t* mem_idx, double abs_tol, env_radius_fn fn,
                             void* user, uint64_t* outer, int32_t* status, int32_t* nlp) {
    if (d < 1 || d > env::MAX_DIM) return -1;
    for (long long w = 0; w < L; ++w) {
        long long lo = 0, hi = 0;
        bool ok = env::list_bounds(reg_off, env::find_region(reg_off, B, w), w, L, lo, hi);
        for (long long k = lo; ok && k < hi; ++k) ok = env::member_ok(mem_idx ? (long long)mem_idx[k] : k, C, mc, mc_max);
        if (!ok) {
            outer[w] = 0;
            status[w] = env::ENV_UNSUPPORTED;
            nlp[w] = 0;
            continue;
        }
        const long long i = mem_idx ? (long long)mem_idx[w] : w;
        env::Walk s;
        env::begin(s, env::member_rows(mc, mc_max, i));
        HostOracle o{d, mc_max, A, b, mc, mem_idx, lo, w, i, fn, user};
        env::walk(s, hi - lo, w - lo, abs_tol, o);
        if (o.rc) return o.rc;
        unsigned long long out = 0;
        status[w] = env::finish(s, out);
        outer[w] = out;
        nlp[w] = s.nlp;
    }
    return 0;
}

#ifdef ENVELOPE_HOST_MAIN
#include <stdio.h>

#include <map>
#include <tuple>

namespace {

struct Replay {
    int d, mc_max;
    const double *A, *b;
    const int32_t *mc, *mem_idx, *reg_off;
    long long B;
    std::map<std::tuple<long long, long long, int>, double> radius;
    long long asked = 0, missing = 0, wrong_stack = 0;
};

// the radius recorded for (w, j, ii); the stack must be [rows of the partner; -row ii of the owner], bit for bit
int replay_radius(long long w, long long j, int ii, int n, const double* stack, double* R, void* user) {
    Replay& P = *static_cast<Replay*>(user);
    P.asked++;
    const long long p = env::find_region(P.reg_off, P.B, w);
    const long long lo = P.reg_off[p];
    const long long c = P.mem_idx ? P.mem_idx[lo + j] : lo + j, own = P.mem_idx ? P.mem_idx[w] : w;
    bool same = n == env::member_rows(P.mc, P.mc_max, c) + 1;
    for (int r = 0; same && r < n; ++r)
        for (int k = 0; same && k <= P.d; ++k) {
            const long long g = r < n - 1 ? c * P.mc_max + r : own * P.mc_max + ii;
            const double v = k < P.d ? P.A[g * P.d + k] : P.b[g];
            const double want = r < n - 1 ? v : -v;
            same = memcmp(&want, &stack[(size_t)r * (P.d + 1) + k], sizeof(double)) == 0;
        }
    P.wrong_stack += !same;
    const auto it = P.radius.find(std::make_tuple(w, j, ii));
    if (it == P.radius.end()) {
        P.missing++;
        return 99;
    }
    *R = it->second;
    return 0;
}

bool read_doubles(FILE* f, std::vector<double>& v, size_t n) {
    v.resize(n);
    for (size_t i = 0; i < n; ++i)
        if (fscanf(f, "%la", &v[i]) != 1) return false;
    return true;
}
bool read_ints(FILE* f, std::vector<int32_t>& v, size_t n) {
    v.resize(n);
    for (size_t i = 0; i < n; ++i)
        if (fscanf(f, "%d", &v[i]) != 1) return false;
    return true;
}

}  // namespace

// file: n_cases, then per case:  d C mc_max B L has_idx abs_tol(hex) / A / b / mc / reg_off / mem_idx (has_idx) /
// n_radii, then per radius: w j ii radius (hex float or "nan") / per entry: outer (decimal) status nlp
int main(int argc, char** argv) {
    if (argc < 2) return 2;
    FILE* f = fopen(argv[1], "r");
    if (!f) return 2;
    int n_cases = 0;
    if (fscanf(f, "%d", &n_cases) != 1) return 2;
    long long bad = 0, entries = 0, lps = 0;
    for (int t = 0; t < n_cases; ++t) {
        int d, C, mc_max, B, L, has_idx, n_rad;
        double tol;
        if (fscanf(f, "%d %d %d %d %d %d %la", &d, &C, &mc_max, &B, &L, &has_idx, &tol) != 7) return 2;
        std::vector<double> A, b;
        std::vector<int32_t> mc, reg_off, mem_idx;
        if (!read_doubles(f, A, (size_t)C * mc_max * d) || !read_doubles(f, b, (size_t)C * mc_max) || !read_ints(f, mc, C) ||
            !read_ints(f, reg_off, (size_t)B + 1) || !read_ints(f, mem_idx, has_idx ? L : 0))
            return 2;
        Replay P{d, mc_max, A.data(), b.data(), mc.data(), has_idx ? mem_idx.data() : nullptr, reg_off.data(), B};
        if (fscanf(f, "%d", &n_rad) != 1) return 2;
        for (int k = 0; k < n_rad; ++k) {
            long long w, j;
            int ii;
            std::vector<double> r;
            if (fscanf(f, "%lld %lld %d", &w, &j, &ii) != 3 || !read_doubles(f, r, 1)) return 2;
            P.radius[std::make_tuple(w, j, ii)] = r[0];
        }
        std::vector<unsigned long long> want_outer(L);
        std::vector<int32_t> want_status(L), want_nlp(L);
        for (int w = 0; w < L; ++w)
            if (fscanf(f, "%llu %d %d", &want_outer[w], &want_status[w], &want_nlp[w]) != 3) return 2;
        // buffers of exactly the sizes the rule was told: a write past them is the sanitizer's to find
        std::vector<uint64_t> outer(L);
        std::vector<int32_t> status(L), nlp(L);
        const int rc = envelope_host(d, C, mc_max, A.data(), b.data(), mc.data(), B, reg_off.data(), L, P.mem_idx, tol,
                                     replay_radius, &P, outer.data(), status.data(), nlp.data());
        bool ok = rc == 0 && P.missing == 0 && P.wrong_stack == 0;
        for (int w = 0; ok && w < L; ++w) ok = outer[w] == want_outer[w] && status[w] == want_status[w] && nlp[w] == want_nlp[w];
        bad += !ok;
        entries += L;
        lps += P.asked;
    }
    fclose(f);
    printf("envelope_host: %d cases, %lld list entries, %lld LPs, inconsistent: %lld\n", n_cases, entries, lps, bad);
    return bad ? 1 : 0;
}
#endif
