// Host build of polytope_amd/csrc/plp_volume_exact.hpp (the sequential rule of volume_exact_kernel, plp_volume_exact.hip):
// TEST INFRASTRUCTURE, compiled with g++ -ffp-contract=off by tests/volume_exact_host.py.  volume_exact_host is
// plp_vol_exact_batch in a plain loop over volume_exact::one<D> -- the device's answers are held against these bit for
// bit.
//
// -DVOLUME_EXACT_HOST_MAIN adds a main(): a stand-alone program that reads polytopes from a file (int32 count, then per
// polytope int32 m, int32 d, m * d doubles A, m doubles b) and runs the same loop on them with every row live, with a keep
// mask with holes, with a centre and a scale and without the areas, for a run under -fsanitize=address,undefined without
// anything loaded into an interpreter.
#include <stdint.h>

#include <vector>

#include "../../polytope_amd/csrc/plp_volume_exact.hpp"

namespace {

template <int D>
void run_d(long long B, int m_max, const double* A, const double* b, const int* m, const uint64_t* keep, const double* xc,
           const double* scale, double* volume, double* area, int* status) {
    std::vector<double> work(plp::volume_exact::lds_bytes(D, m_max) / sizeof(double) + 1);
    for (long long p = 0; p < B; ++p)
        plp::volume_exact::one<D>(m_max, A + (size_t)p * m_max * D, b + (size_t)p * m_max, m ? m[p] : m_max,
                                  keep ? keep[p] : ~(uint64_t)0, xc ? xc + (size_t)p * D : nullptr, scale ? scale[p] : 1.0,
                                  volume[p], area ? area + (size_t)p * m_max : nullptr, status[p], work.data());
}

}  // namespace

// the arguments of plp_vol_exact_batch without the context; 0, or 2 for a size the kernel does not take
extern "C" int volume_exact_host(long long B, int m_max, int d, const double* A, const double* b, const int* m,
                                 const uint64_t* keep, const double* xc, const double* scale, double* volume, double* area,
                                 int* status) {
    if (B < 1 || m_max < 0 || m_max > plp::wenum::MAX_ITEMS) return 2;
    return plp::wenum::dispatch_dim(
        d, [&](auto dim) { run_d<decltype(dim)::value>(B, m_max, A, b, m, keep, xc, scale, volume, area, status); });
}

#ifdef VOLUME_EXACT_HOST_MAIN
#include <stdio.h>

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    int32_t ncase = 0;
    if (fread(&ncase, sizeof(ncase), 1, f) != 1) return 2;
    long long ok = 0, unbounded = 0, empty = 0, bad = 0;
    for (int32_t c = 0; c < ncase; ++c) {
        int32_t md[2];
        if (fread(md, sizeof(int32_t), 2, f) != 2) return 2;
        const int m = md[0], d = md[1];
        std::vector<double> A((size_t)m * d), b(m);
        if (fread(A.data(), sizeof(double), A.size(), f) != A.size() || fread(b.data(), sizeof(double), b.size(), f) != b.size())
            return 2;
        const uint64_t holes = 0xb6db6db6db6db6dbull;   // two rows of three
        const double xc[4] = {0.25, -0.5, 0.125, 1.0}, scale = 2.0;
        double first = 0.0;
        for (int pass = 0; pass < 4; ++pass) {
            const uint64_t keep = pass == 1 ? holes : ~(uint64_t)0;
            std::vector<double> area(m > 0 ? m : 1, -1.0);
            double volume = -1.0;
            int status = -1, mm = m;
            if (volume_exact_host(1, m, d, A.data(), b.data(), &mm, &keep, pass == 2 ? xc : nullptr, pass == 2 ? &scale : nullptr,
                                  &volume, pass == 3 ? nullptr : area.data(), &status) != 0) { ++bad; continue; }
            bad += status < 0 || status > 2 || !(volume == volume) || (status == 1) != (volume == __builtin_inf()) ||
                   (status == 2 && volume != 0.0);
            for (int i = 0; i < m && pass != 3; ++i) bad += !(area[i] == area[i]);
            if (pass == 0) first = volume;
            if (pass == 3) bad += volume != first;   // the areas change nothing else
            if (pass == 0) { ok += status == 0; unbounded += status == 1; empty += status == 2; }
        }
    }
    fclose(f);
    printf("volume_exact_host: %d polytopes x 4 passes, %lld ok, %lld unbounded, %lld empty, inconsistent: %lld\n", (int)ncase, ok,
           unbounded, empty, bad);
    return bad ? 1 : 0;
}
#endif
