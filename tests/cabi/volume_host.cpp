// Host build of polytope_amd/csrc/plp_volume.hpp (the generator, the sample and the row test of the Monte-Carlo volume
// kernel, plp_volume.hip): TEST INFRASTRUCTURE, compiled with g++ -ffp-contract=off by tests/volume_host.py.  vh_hits is the
// whole sample-and-test loop over a packed batch, written the plain way -- d generator states per polytope, state k
// started at stream position k * N by pcg64_advance and stepped once per sample -- so that the kernel's walk (one state,
// jumps of N and of the workgroup's width) is held against a second route through the same stream.
#include <stdint.h>

#include "../../polytope_amd/csrc/plp_volume.hpp"

using plp::vol::u128;

namespace {

template <int D>
void hits_d(long long B, int m_max, const double* A, const double* b, const int* m, const double* lb, const double* ub,
            const uint64_t* state, const uint64_t* inc, long long N, uint32_t* hits, int* flags) {
#pragma omp parallel for schedule(dynamic, 8)
    for (long long p = 0; p < B; ++p) {
        int mk = m ? m[p] : m_max;
        mk = mk < 0 ? 0 : (mk > m_max ? m_max : mk);
        double lo[D], wd[D];
        bool finite = true;
        for (int k = 0; k < D; ++k) {
            lo[k] = lb[p * D + k];
            wd[k] = ub[p * D + k] - lo[k];
            finite = finite && isfinite(lo[k]) && isfinite(ub[p * D + k]);
        }
        hits[p] = 0;
        flags[p] = (finite ? 0 : plp::vol::VF_NONFINITE) | (mk == 0 ? plp::vol::VF_NOROWS : 0);
        if (flags[p]) continue;
        const u128 ic{inc[2 * p], inc[2 * p + 1]};
        u128 s[D];
        for (int k = 0; k < D; ++k)
            s[k] = plp::vol::pcg64_advance(u128{state[2 * p], state[2 * p + 1]}, ic, (uint64_t)k * (uint64_t)N);
        const double* Ap = A + (size_t)p * m_max * D;
        const double* bp = b + (size_t)p * m_max;
        uint32_t cnt = 0;
        for (long long j = 0; j < N; ++j) {
            double x[D];
            for (int k = 0; k < D; ++k) {
                s[k] = plp::vol::pcg64_step(s[k], ic);
                x[k] = plp::vol::sample_coord(lo[k], wd[k], plp::vol::pcg64_double(plp::vol::pcg64_out(s[k])));
            }
            bool in = true;
            for (int i = 0; i < mk && in; ++i) in = plp::vol::row_inside<D>(Ap + i * D, bp[i], x);
            cnt += in ? 1u : 0u;
        }
        hits[p] = cnt;
    }
}

}  // namespace

extern "C" {

// out[i] = the i-th double of the stream, i < count (numpy: default_rng(seed).random(count))
void vh_stream(const uint64_t* state, const uint64_t* inc, long long count, double* out) {
    u128 s{state[0], state[1]};
    const u128 ic{inc[0], inc[1]};
    for (long long i = 0; i < count; ++i) {
        s = plp::vol::pcg64_step(s, ic);
        out[i] = plp::vol::pcg64_double(plp::vol::pcg64_out(s));
    }
}

// out[i] = (low, high) of the state after n[i] steps; jump != 0: through pcg64_jump + pcg64_apply (the kernel's constants)
void vh_advance(const uint64_t* state, const uint64_t* inc, long long count, const uint64_t* n, int jump, uint64_t* out) {
    const u128 s{state[0], state[1]}, ic{inc[0], inc[1]};
    for (long long i = 0; i < count; ++i) {
        const u128 r = jump ? plp::vol::pcg64_apply(plp::vol::pcg64_jump(n[i]), s, ic) : plp::vol::pcg64_advance(s, ic, n[i]);
        out[2 * i] = r.lo;
        out[2 * i + 1] = r.hi;
    }
}

// out[i] = the double at stream position pos[i], reached directly
void vh_at(const uint64_t* state, const uint64_t* inc, long long count, const uint64_t* pos, double* out) {
    const u128 s{state[0], state[1]}, ic{inc[0], inc[1]};
    for (long long i = 0; i < count; ++i)
        out[i] = plp::vol::pcg64_double(plp::vol::pcg64_out(plp::vol::pcg64_advance(s, ic, pos[i] + 1)));
}

int vh_hits(long long B, int m_max, int d, const double* A, const double* b, const int* m, const double* lb,
            const double* ub, const uint64_t* state, const uint64_t* inc, long long N, uint32_t* hits, int* flags) {
    if (d < 1 || d > 16 || m_max < 0 || m_max > 64 || N < 1 || N > 0x7fffffffll) return 2;
#define VH_CASE(K) case K: hits_d<K>(B, m_max, A, b, m, lb, ub, state, inc, N, hits, flags); break;
    switch (d) {
        VH_CASE(1) VH_CASE(2) VH_CASE(3) VH_CASE(4) VH_CASE(5) VH_CASE(6) VH_CASE(7) VH_CASE(8) VH_CASE(9) VH_CASE(10)
        VH_CASE(11) VH_CASE(12) VH_CASE(13) VH_CASE(14) VH_CASE(15) VH_CASE(16)
    }
#undef VH_CASE
    return 0;
}

}  // extern "C"
