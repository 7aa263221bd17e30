// Host build of polytope_amd/csrc/plp_extreme.hpp (the sequential rule of extreme_kernel, plp_extreme.hip): TEST
// INFRASTRUCTURE, compiled with g++ -ffp-contract=off by tests/extreme_host.py.  extreme_host is plp_extreme_batch in a
// plain loop over extreme::one<D> -- the device's answers are held against these bit for bit.
//
// -DEXTREME_HOST_MAIN adds a main(): a stand-alone program that reads polytopes from a file (int32 count, then per
// polytope int32 m, int32 d, m * d doubles A, m doubles b) and runs the same loop on them with every row live, with a
// keep mask with holes, with a v_max of 3 and without the basis, for a run under -fsanitize=address,undefined without
// anything loaded into an interpreter.
#include <stdint.h>

#include "../../polytope_amd/csrc/plp_extreme.hpp"

namespace {

template <int D>
void run_d(long long B, int m_max, const double* A, const double* b, const int* m, const uint64_t* keep, int v_max, double* V,
           int* count, int* basis, int* status) {
    for (long long p = 0; p < B; ++p) {
        const size_t slot = (size_t)p * v_max * D;
        plp::extreme::one<D>(m_max, A + (size_t)p * m_max * D, b + (size_t)p * m_max, m ? m[p] : m_max,
                             keep ? keep[p] : ~(uint64_t)0, v_max, V + slot, basis ? basis + slot : nullptr, count[p], status[p]);
    }
}

}  // namespace

// the arguments of plp_extreme_batch without the context; 0, or 2 for a size the kernel does not take
extern "C" int extreme_host(long long B, int m_max, int d, const double* A, const double* b, const int* m, const uint64_t* keep,
                            int v_max, double* V, int* count, int* basis, int* status) {
    if (m_max < 0 || m_max > plp::wenum::MAX_ITEMS || v_max < 1) return 2;
    return plp::wenum::dispatch_dim(
        d, [&](auto dim) { run_d<decltype(dim)::value>(B, m_max, A, b, m, keep, v_max, V, count, basis, status); });
}

namespace {
template <int D>
long long unrank_mismatches() {
    long long bad = 0;
    for (int n = D; n <= plp::wenum::MAX_ITEMS; ++n) {
        int idx[D], got[D];
        for (int k = 0; k < D; ++k) idx[k] = k;
        int r = 0;
        do {
            plp::wenum::unrank<D>(n, r, got);
            for (int k = 0; k < D; ++k) bad += got[k] != idx[k];
            ++r;
        } while (plp::wenum::next<D>(n, idx));
        bad += r != plp::wenum::candidates<D>(n);
    }
    return bad;
}
}  // namespace

// unrank() against next() (plp_enum.hpp) on every subset of every n <= 64: the number of mismatches (-1: d not in 1 .. 4)
extern "C" long long extreme_unrank_mismatches(int d) {
    long long bad = -1;
    plp::wenum::dispatch_dim(d, [&](auto dim) { bad = unrank_mismatches<decltype(dim)::value>(); });
    return bad;
}

#ifdef EXTREME_HOST_MAIN
#include <stdio.h>

#include <vector>

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    int32_t ncase = 0;
    if (fread(&ncase, sizeof(ncase), 1, f) != 1) return 2;
    long long vertices = 0, overflow = 0, empty = 0, bad = 0;
    for (int32_t c = 0; c < ncase; ++c) {
        int32_t md[2];
        if (fread(md, sizeof(int32_t), 2, f) != 2) return 2;
        const int m = md[0], d = md[1];
        std::vector<double> A((size_t)m * d), b(m);
        if (fread(A.data(), sizeof(double), A.size(), f) != A.size() || fread(b.data(), sizeof(double), b.size(), f) != b.size())
            return 2;
        const int full = d == 1 ? 2 : (d == 2 ? m : (d == 3 ? 2 * m - 4 : m * (m - 3) / 2));
        const uint64_t holes = 0xb6db6db6db6db6dbull;   // two rows of three
        for (int pass = 0; pass < 4; ++pass) {
            const int v_max = pass == 2 ? 3 : (full > 1 ? full : 1);
            const uint64_t keep = pass == 1 ? holes : ~(uint64_t)0;
            std::vector<double> V((size_t)v_max * d);
            std::vector<int> basis((size_t)v_max * d);
            int count = -1, status = -1, mm = m;
            if (extreme_host(1, m, d, A.data(), b.data(), &mm, &keep, v_max, V.data(), &count, pass == 3 ? nullptr : basis.data(),
                             &status) != 0) { ++bad; continue; }
            bad += count < 0 || count > v_max || status < 0 || status > 2 || (status == 2) != (count == 0);
            for (int q = 0; q < count * d; ++q) bad += !(V[q] == V[q]) || (pass != 3 && (basis[q] < 0 || basis[q] >= m));
            for (int q = count * d; q < v_max * d; ++q) bad += V[q] == V[q];
            vertices += count; overflow += status == 1; empty += status == 2;
        }
    }
    fclose(f);
    printf("extreme_host: %d polytopes x 4 passes, %lld vertices, %lld overflows, %lld empty, inconsistent: %lld\n", (int)ncase,
           vertices, overflow, empty, bad);
    return bad ? 1 : 0;
}
#endif
