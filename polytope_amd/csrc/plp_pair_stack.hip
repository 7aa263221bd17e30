// plp_pair_stack.hip -- the stacks of listed cell pairs of a resident table, formed on the device (gfx950): the rule is
// plp_pair_stack.hpp, the reference forms each stack as a Python object (polytope/polytope.py:272-275).
//
//   pair_stack_kernel<D> : ONE LANE PER ROW SLOT, floor(64 / W) STACKS PER WAVEFRONT (W = 2 m_max row slots per stack).
//                          Lane l of a wavefront serves slot s = l % W of the wavefront's stack g = l / W: 4 stacks at
//                          W = 16, 2 at W = 32 (or 24), 1 at W = 64; the 64 % W lanes left over idle.  A lane loads its
//                          table row (the rows of a cell are one contiguous run, and neighbouring lanes hold neighbouring
//                          rows: the D loads of a wavefront cover whole lines between them), runs the constructor pass in
//                          registers (fm::scale<D>), and one ballot gives every kept row its slot: the popcount of its
//                          stack's segment of the mask below it.  Kept rows are written at their slot, lanes whose own
//                          index is >= ms write the zero rows, so every slot of a stack is written exactly once.  No LDS,
//                          no scratch.  The kernel moves (D + 1) * 8 bytes in and out per row for 2 D + 2 flops: its
//                          bound is memory.  NOT MEASURED -- see DESIGN 4.21.
//   pair_bad_kernel      : one lane per pair of a chunk of plp_intersect_pairs_dev, after its reduce and emission: a bad
//                          pair (plp_pair_index.hpp) gets PLP_RF_EMPTY | PLP_RF_BADPAIR and outputs that do not depend
//                          on what the reduce made of an empty stack.
#include "plp_pair_stack.hpp"
#include "plp_common.hpp"
#include "plp_kernels.hpp"

namespace plp {
namespace {

constexpr int PS_BLOCK = 256;   // four wavefronts

template <int D>
__global__ __launch_bounds__(PS_BLOCK) void pair_stack_kernel(int n, int m_max, const double* __restrict__ A,
                                                              const double* __restrict__ b, const int* __restrict__ m,
                                                              long long K, const int* __restrict__ pairs,
                                                              double* __restrict__ A_s, double* __restrict__ b_s,
                                                              int* __restrict__ m_s) {
    const int W = 2 * m_max;
    const int G = 64 / W;                       // stacks per wavefront
    const int lane = threadIdx.x & 63;
    const int g = lane / W, s = lane - g * W;   // this lane's stack of the wavefront and its row slot
    const bool active = g < G;
    const unsigned long long seg_mask = W == 64 ? ~0ull : ((1ull << W) - 1ull);
    const long long waves = (long long)gridDim.x * (PS_BLOCK / 64);
    const long long wave0 = (long long)blockIdx.x * (PS_BLOCK / 64) + (threadIdx.x >> 6);
    for (long long t0 = wave0 * G; t0 < K; t0 += waves * G) {   // (wave-uniform bounds: every lane reaches the ballot)
        const long long t = t0 + g;
        const bool mine = active && t < K;
        long long i, j;
        const bool ok = pair_cells<true>(t, mine, n, 0, pairs, i, j);
        const int mi = ok ? ps::cell_rows(m, i, m_max) : 0, mj = ok ? ps::cell_rows(m, j, m_max) : 0;
        const long long row = ps::source_row(i, j, mi, mj, m_max, s);
        double x[D];
        double bb = 0.0;
        bool kept = false;
        if (ok && row >= 0) kept = ps::stack_row<D>(A, b, row, x, bb);
        const unsigned long long seg = (__ballot(kept) >> (g * W)) & seg_mask;
        if (!mine) continue;
        const int ms = __popcll(seg);
        const int pos = __popcll(seg & ((1ull << s) - 1ull));
        double* Ao = A_s + (size_t)t * W * D;
        double* bo = b_s + (size_t)t * W;
        if (kept) {
#pragma unroll
            for (int c = 0; c < D; ++c) Ao[(size_t)pos * D + c] = x[c];
            bo[pos] = bb;
        }
        if (s >= ms) {
#pragma unroll
            for (int c = 0; c < D; ++c) Ao[(size_t)s * D + c] = 0.0;
            bo[s] = 0.0;
        }
        if (s == 0) m_s[t] = ms;
    }
}

__global__ __launch_bounds__(PS_BLOCK) void pair_bad_kernel(int n, int d, long long K, const int* __restrict__ pairs,
                                                            unsigned long long* __restrict__ keep, int* __restrict__ flags,
                                                            double* __restrict__ r, double* __restrict__ xc,
                                                            int* __restrict__ nlp, int* __restrict__ ms,
                                                            int* __restrict__ m_out) {
    const long long t = (long long)blockIdx.x * PS_BLOCK + threadIdx.x;
    if (t >= K) return;
    long long i, j;
    if (pair_cells<true>(t, true, n, 0, pairs, i, j)) return;
    keep[t] = 0ull;
    flags[t] = RF_EMPTY | RF_BADPAIR;
    r[t] = 0.0;
    for (int c = 0; c < d; ++c) xc[(size_t)t * d + c] = __builtin_nan("");
    nlp[t] = 0;
    ms[t] = 0;
    if (m_out) m_out[t] = 0;
}

template <int D>
void launch_t(int n, int m_max, const double* A, const double* b, const int* m, long long K, const int* pairs, double* A_s,
              double* b_s, int* m_s, hipStream_t st) {
    const long long per_block = (long long)(PS_BLOCK / 64) * (64 / (2 * m_max));
    long long grid = (K + per_block - 1) / per_block;
    if (grid > (1ll << 20)) grid = 1ll << 20;   // (the kernel strides over the rest)
    hipLaunchKernelGGL(pair_stack_kernel<D>, dim3((unsigned)grid), dim3(PS_BLOCK), 0, st, n, m_max, A, b, m, K, pairs, A_s, b_s,
                       m_s);
}

}  // namespace

int launch_pair_stacks(int n, int m_max, int d, const double* A, const double* b, const int* m, long long K, const int* pairs,
                       double* A_s, double* b_s, int* m_s, hipStream_t st) {
    if (n < 0 || m_max < 1 || 2 * m_max > ps::MAX_W || K < 0) return 2;
    if (K == 0) return 0;
#define PLP_PS_CASE(DD) \
    case DD: launch_t<DD>(n, m_max, A, b, m, K, pairs, A_s, b_s, m_s, st); return 0;
    switch (d) {
        PLP_PS_CASE(1) PLP_PS_CASE(2) PLP_PS_CASE(3) PLP_PS_CASE(4) PLP_PS_CASE(5) PLP_PS_CASE(6) PLP_PS_CASE(7)
        PLP_PS_CASE(8) PLP_PS_CASE(9) PLP_PS_CASE(10) PLP_PS_CASE(11) PLP_PS_CASE(12) PLP_PS_CASE(13) PLP_PS_CASE(14)
        PLP_PS_CASE(15) PLP_PS_CASE(16)
        default: return 2;
    }
#undef PLP_PS_CASE
}

void launch_pair_bad(int n, int d, long long K, const int* pairs, unsigned long long* keep, int* flags, double* r, double* xc,
                     int* nlp, int* ms, int* m_out, hipStream_t st) {
    if (K <= 0) return;
    hipLaunchKernelGGL(pair_bad_kernel, dim3((unsigned)((K + PS_BLOCK - 1) / PS_BLOCK)), dim3(PS_BLOCK), 0, st, n, d, K, pairs,
                       keep, flags, r, xc, nlp, ms, m_out);
}

}  // namespace plp
