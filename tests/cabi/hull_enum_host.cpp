// Host build of polytope_amd/csrc/plp_hull_enum.hpp (the sequential rule of hull_enum_kernel, plp_hull_enum.hip): TEST
// INFRASTRUCTURE, compiled with g++ -ffp-contract=off by tests/hull_host.py.  hull_enum_host is plp_hull_batch in a plain
// loop over hullenum::one<D> -- the device's answers are held against these bit for bit.
//
// -DHULL_HOST_MAIN adds a main(): a stand-alone program that reads point sets from a file (int32 count, then per set
// int32 n, int32 d, n * d doubles), packs the sets of one dimension into ONE ragged batch and runs the same loop on it with
// every point live, with a keep mask with holes, with an f_max of 3 and without the basis, for a run under
// -fsanitize=address,undefined without anything loaded into an interpreter.
#include <stdint.h>

#include "../../polytope_amd/csrc/plp_hull_enum.hpp"

namespace {

template <int D>
void run_d(long long B, int n_max, const double* X, const int* n, const uint64_t* keep, int f_max, double* Ao, double* bo,
           uint64_t* on, int* count, int* basis, int* status) {
    for (long long p = 0; p < B; ++p) {
        const size_t slot = (size_t)p * f_max;
        plp::hullenum::one<D>(n_max, X + (size_t)p * n_max * D, n ? n[p] : n_max, keep ? keep[p] : ~(uint64_t)0, f_max,
                              Ao + slot * D, bo + slot, on + slot, basis ? basis + slot * D : nullptr, count[p], status[p]);
    }
}

}  // namespace

// the arguments of plp_hull_batch without the context; 0, or 2 for a size the kernel does not take
extern "C" int hull_enum_host(long long B, int n_max, int d, const double* X, const int* n, const uint64_t* keep, int f_max,
                              double* Ao, double* bo, uint64_t* on, int* count, int* basis, int* status) {
    if (n_max < 0 || n_max > plp::wenum::MAX_ITEMS || f_max < 1) return 2;
    return plp::wenum::dispatch_dim(
        d, [&](auto dim) { run_d<decltype(dim)::value>(B, n_max, X, n, keep, f_max, Ao, bo, on, count, basis, status); });
}

#ifdef HULL_HOST_MAIN
#include <stdio.h>

#include <vector>

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    int32_t ncase = 0;
    if (fread(&ncase, sizeof(ncase), 1, f) != 1) return 2;
    std::vector<std::vector<double>> pts[5];
    for (int32_t c = 0; c < ncase; ++c) {
        int32_t nd[2];
        if (fread(nd, sizeof(int32_t), 2, f) != 2) return 2;
        if (nd[0] < 0 || nd[0] > 64 || nd[1] < 1 || nd[1] > 4) return 2;
        std::vector<double> x((size_t)nd[0] * nd[1]);
        if (!x.empty() && fread(x.data(), sizeof(double), x.size(), f) != x.size()) return 2;
        pts[nd[1]].push_back(x);
    }
    fclose(f);
    long long facets = 0, overflow = 0, flat = 0, bad = 0, sets = 0;
    for (int d = 1; d <= 4; ++d) {
        const long long B = (long long)pts[d].size();
        if (!B) continue;
        int n_max = 0;
        std::vector<int> n(B);
        for (long long p = 0; p < B; ++p) {
            n[p] = (int)(pts[d][p].size() / d);
            n_max = n[p] > n_max ? n[p] : n_max;
        }
        std::vector<double> X((size_t)B * n_max * d, 0.0);
        for (long long p = 0; p < B; ++p)
            for (size_t q = 0; q < pts[d][p].size(); ++q) X[(size_t)p * n_max * d + q] = pts[d][p][q];
        const int full = d == 1 ? 2 : (d == 2 ? n_max : (d == 3 ? 2 * n_max - 4 : n_max * (n_max - 3) / 2));
        std::vector<uint64_t> holes(B, 0xb6db6db6db6db6dbull);   // two points of three
        sets += B;
        for (int pass = 0; pass < 4; ++pass) {
            const int f_max = pass == 2 ? 3 : (full > 1 ? full : 1);
            std::vector<double> Ao((size_t)B * f_max * d), bo((size_t)B * f_max);
            std::vector<uint64_t> on((size_t)B * f_max);
            std::vector<int> basis((size_t)B * f_max * d), count(B, -1), status(B, -1);
            if (hull_enum_host(B, n_max, d, X.data(), n.data(), pass == 1 ? holes.data() : nullptr, f_max, Ao.data(), bo.data(),
                               on.data(), count.data(), pass == 3 ? nullptr : basis.data(), status.data()) != 0) { ++bad; continue; }
            for (long long p = 0; p < B; ++p) {
                const int cnt = count[p];
                bad += cnt < 0 || cnt > f_max || status[p] < 0 || status[p] > 2 || (status[p] == 2) != (cnt == 0);
                if (cnt < 0 || cnt > f_max) continue;
                const size_t s0 = (size_t)p * f_max;
                for (int q = 0; q < f_max; ++q) {
                    const bool in = q < cnt;
                    bad += (bo[s0 + q] == bo[s0 + q]) != in || (on[s0 + q] != 0) != in;
                    for (int k = 0; k < d; ++k) {
                        const double a = Ao[(s0 + q) * d + k];
                        bad += (a == a) != in;
                        if (pass != 3) bad += in ? (basis[(s0 + q) * d + k] < 0 || basis[(s0 + q) * d + k] >= n[p]) : basis[(s0 + q) * d + k] != -1;
                    }
                }
                facets += cnt; overflow += status[p] == 1; flat += status[p] == 2;
            }
        }
    }
    printf("hull_enum_host: %lld point sets x 4 passes, %lld facets, %lld overflows, %lld flat, inconsistent: %lld\n", sets, facets,
           overflow, flat, bad);
    return bad ? 1 : 0;
}
#endif
