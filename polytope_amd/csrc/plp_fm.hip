// plp_fm.hip -- one Fourier-Motzkin elimination step for a batch of packed polytopes (reference: projection_fm,
// polytope/polytope.py:1911-1952), fused with the compaction of the reduce() that produced its input rows.
//
// One wavefront per polytope.  Stage: the rows the keep words mark go through what the host would do to them
// (plp_fm.hpp: stage) and land, compacted, in LDS as [row][d + 1] (b last); P / Q / N position lists are built by ballot
// and prefix popcount over chunks of 64 rows, so inputs of any row count the LDS holds (the wide reduce's) are read in
// chunks.  Count: |N| + |P| |Q|.  Emit: candidate output rows are striped over the lanes 64 at a time, in the reference's
// order (P x Q, j major, then N), and the rows that survive the scaling are written at their prefix position.
//
// col < 0: no elimination -- the staged rows are written as they are (the compaction of the last step's reduce).
#include "plp_fm.hpp"
#include "plp_common.hpp"
#include "plp_kernels.hpp"

namespace plp {
namespace {

struct FmArgs {
    long long B;
    int m_max, col, first, mo_max, kw;
    const double* A;
    const double* b;
    const int* m;
    const unsigned long long* keep;
    const int* flags;
    double abs_tol;
    int* count;
    double* Aout;
    double* bout;
    int* mout;
};

constexpr int FM_DEAD = RF_EMPTY | RF_LPFAIL | RF_F1OPEN;

__device__ __forceinline__ int lanes_below(unsigned long long mask) {
    return __builtin_amdgcn_mbcnt_hi((unsigned)(mask >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mask, 0u));
}

// LDS of one workgroup (one wavefront): rows [m_max][D + 1], then three int lists [m_max]
template <int D>
__host__ __device__ constexpr size_t fm_lds_bytes_t(int m_max) {
    return (size_t)m_max * (D + 1) * 8 + (size_t)3 * m_max * 4;
}

template <int D, bool ELIM, bool EMIT>
__global__ __launch_bounds__(64) void fm_kernel(FmArgs a) {
    extern __shared__ double fm_lds[];
    constexpr int S = D + 1;
    constexpr int DO = ELIM ? D - 1 : D;
    double* rows = fm_lds;
    int* lst = reinterpret_cast<int*>(fm_lds + (size_t)a.m_max * S);   // P | Q | N, m_max each
    int* lP = lst;
    int* lQ = lst + a.m_max;
    int* lN = lst + 2 * a.m_max;
    const int lane = threadIdx.x;
    for (long long p = blockIdx.x; p < a.B; p += gridDim.x) {
        int mk = a.m ? a.m[p] : a.m_max;
        mk = mk < 0 ? 0 : (mk > a.m_max ? a.m_max : mk);
        const int fl = a.flags ? a.flags[p] : 0;
        if (fl & FM_DEAD) mk = 0;   // empty / failed / to be re-examined on the host: nothing to emit
        const bool shift = (fl & RF_MINREP) != 0;
        const int passes = (a.flags ? 1 : 0) + (a.first ? 1 : 0);
        const double* Ap = a.A + (size_t)p * a.m_max * D;
        const double* bp = a.b + (size_t)p * a.m_max;
        const unsigned long long* kp = a.keep ? a.keep + (size_t)p * a.kw : nullptr;
        int nv = 0, nP = 0, nQ = 0, nN = 0;
        for (int base = 0; base < mk; base += 64) {
            const int r = base + lane;
            bool ok = r < mk;
            if (ok && kp) ok = ((kp[r >> 6] >> (r & 63)) & 1ull) != 0;
            double x[D];
            double bb = 0.0;
            if (ok) {
#pragma unroll
                for (int c = 0; c < D; ++c) x[c] = Ap[(size_t)r * D + c];
                bb = bp[r];
                ok = fm::stage<D>(x, bb, shift, passes);
            }
            int cls = fm::CLS_NONE;
            if (ok) cls = ELIM ? fm::classify(fm::pick<D>(x, a.col), a.abs_tol) : fm::CLS_N;
            const unsigned long long mv = __ballot(ok);
            const unsigned long long mP = __ballot(ok && cls == fm::CLS_P);
            const unsigned long long mQ = __ballot(ok && cls == fm::CLS_Q);
            const unsigned long long mN = __ballot(ok && cls == fm::CLS_N);
            if constexpr (EMIT) {   // (the count needs the three sizes only)
                const int pos = nv + lanes_below(mv);
                if (ok) {
#pragma unroll
                    for (int c = 0; c < D; ++c) rows[pos * S + c] = x[c];
                    rows[pos * S + D] = bb;
                }
                if (ok && cls == fm::CLS_P) lP[nP + lanes_below(mP)] = pos;
                if (ok && cls == fm::CLS_Q) lQ[nQ + lanes_below(mQ)] = pos;
                if (ok && cls == fm::CLS_N) lN[nN + lanes_below(mN)] = pos;
            }
            nv += __popcll(mv);
            nP += __popcll(mP);
            nQ += __popcll(mQ);
            nN += __popcll(mN);
        }
        __syncthreads();   // (one wavefront per workgroup: orders the LDS writes above before the reads below)
        const long long npq = (long long)nP * nQ;
        const long long cnt = npq + nN;
        if constexpr (!EMIT) {
            if (lane == 0) a.count[p] = cnt > 0x7fffffffll ? 0x7fffffff : (int)cnt;
        } else {
            double* Ao = a.Aout + (size_t)p * a.mo_max * DO;
            double* bo = a.bout + (size_t)p * a.mo_max;
            int out_n = 0;
            if (cnt > a.mo_max) {
                out_n = -1;   // does not fit the output: the host takes this polytope (no row written)
            } else {
                for (long long t0 = 0; t0 < cnt; t0 += 64) {
                    const long long t = t0 + lane;
                    bool ok = t < cnt;
                    double y[DO > 0 ? DO : 1];
                    double yb = 0.0;
                    if (ok) {
                        if constexpr (ELIM) {
                            if (t < npq) {
                                const int j = lP[t / nQ], k = lQ[t % nQ];
                                ok = fm::combine<D>(rows + j * S, rows[j * S + D], rows + k * S, rows[k * S + D], a.col, y,
                                                    yb);
                            } else {
                                const int j = lN[t - npq];
                                ok = fm::pass_through<D>(rows + j * S, rows[j * S + D], a.col, y, yb);
                            }
                        } else {
                            const int j = lN[t];
#pragma unroll
                            for (int c = 0; c < D; ++c) y[c] = rows[j * S + c];
                            yb = rows[j * S + D];
                        }
                    }
                    const unsigned long long mv = __ballot(ok);
                    const int pos = out_n + lanes_below(mv);
                    if (ok) {
#pragma unroll
                        for (int c = 0; c < DO; ++c) Ao[(size_t)pos * DO + c] = y[c];
                        bo[pos] = yb;
                    }
                    out_n += __popcll(mv);
                }
                for (int r = out_n + lane; r < a.mo_max; r += 64) {   // zero padding: the reduce reads m[], not these
#pragma unroll
                    for (int c = 0; c < DO; ++c) Ao[(size_t)r * DO + c] = 0.0;
                    bo[r] = 0.0;
                }
            }
            if (lane == 0) a.mout[p] = out_n;
        }
        __syncthreads();   // the next polytope overwrites the LDS
    }
}

template <int D, bool ELIM, bool EMIT>
int launch_fm_t(const FmArgs& a, hipStream_t st) {
    const size_t smem = EMIT ? fm_lds_bytes_t<D>(a.m_max < 1 ? 1 : a.m_max) : 0;
    if (fm_lds_bytes_t<D>(a.m_max < 1 ? 1 : a.m_max) > 160 * 1024) return 2;   // (the emit that follows must fit)
    auto k = fm_kernel<D, ELIM, EMIT>;
    if (smem > 48 * 1024)
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(k), hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
    // workgroups resident per CU at this LDS size, 256 CUs, a few rounds of the grid-stride loop at most
    const long long per_cu = (long long)((160 * 1024) / (smem < 1024 ? 1024 : smem));
    long long grid = 256 * (per_cu < 1 ? 1 : (per_cu > 32 ? 32 : per_cu)) * 4;
    if (grid > a.B) grid = a.B;
    hipLaunchKernelGGL(k, dim3((unsigned)grid), dim3(64), smem, st, a);
    return 0;
}

template <bool EMIT>
int launch_fm_d(int d, const FmArgs& a, hipStream_t st) {
    const bool elim = a.col >= 0;
    if (elim && (d < 2 || a.col >= d)) return 2;
#define PLP_FM_CASE(DD)                                                                      \
    case DD:                                                                                 \
        if constexpr (DD >= 2) {                                                             \
            if (elim) return launch_fm_t<DD, true, EMIT>(a, st);                             \
        }                                                                                    \
        return launch_fm_t<DD, false, EMIT>(a, st);
    switch (d) {
        PLP_FM_CASE(1) PLP_FM_CASE(2) PLP_FM_CASE(3) PLP_FM_CASE(4) PLP_FM_CASE(5) PLP_FM_CASE(6) PLP_FM_CASE(7)
        PLP_FM_CASE(8) PLP_FM_CASE(9) PLP_FM_CASE(10) PLP_FM_CASE(11) PLP_FM_CASE(12) PLP_FM_CASE(13) PLP_FM_CASE(14)
        PLP_FM_CASE(15) PLP_FM_CASE(16)
        default: return 2;
    }
#undef PLP_FM_CASE
}

}  // namespace

size_t fm_lds_bytes(int m_max, int d) { return (size_t)(m_max < 1 ? 1 : m_max) * (d + 1) * 8 + (size_t)3 * (m_max < 1 ? 1 : m_max) * 4; }

int launch_fm(int emit, long long B, int m_max, int d, const double* A, const double* b, const int* mrows,
              const unsigned long long* keep, int kw, const int* flags, int col, int first, double abs_tol, int* count,
              int mo_max, double* Aout, double* bout, int* mout, hipStream_t st) {
    if (B <= 0) return 0;
    FmArgs a{B, m_max, col, first, mo_max, kw, A, b, mrows, keep, flags, abs_tol, count, Aout, bout, mout};
    return emit ? launch_fm_d<true>(d, a, st) : launch_fm_d<false>(d, a, st);
}

}  // namespace plp
