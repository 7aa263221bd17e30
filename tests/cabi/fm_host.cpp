// Host build of polytope_amd/csrc/plp_fm.hpp (the row arithmetic of the Fourier-Motzkin step kernels, plp_fm.hip):
// TEST INFRASTRUCTURE, compiled with g++ -ffp-contract=off by tests/test_projection.py.  fm_step runs one step over a
// packed batch the way the kernels do -- stage the kept rows, split them on column col, emit P x Q then N -- so that its
// output can be held against a numpy statement of the same formula (CPU) and against the device (GPU), bit for bit.
#include <stdint.h>

#include "../../polytope_amd/csrc/plp_fm.hpp"

namespace {

template <int D, bool ELIM>
void step(long long B, int m_max, const double* A, const double* b, const int* m, const uint64_t* keep, int kw,
          const int* flags, int col, int first, double tol, int mo_max, int* count, double* Aout, double* bout, int* mout) {
    constexpr int DO = ELIM ? D - 1 : D;
    static double rows[4096 * (D + 1)];
    static int lP[4096], lQ[4096], lN[4096];
    for (long long p = 0; p < B; ++p) {
        int mk = m ? m[p] : m_max;
        const int fl = flags ? flags[p] : 0;
        if (fl & (1 | 8 | 32)) mk = 0;
        const bool shift = (fl & 4) != 0;
        const int passes = (flags ? 1 : 0) + (first ? 1 : 0);
        int nv = 0, nP = 0, nQ = 0, nN = 0;
        for (int r = 0; r < mk && r < 4096; ++r) {
            if (keep && !((keep[(size_t)p * kw + (r >> 6)] >> (r & 63)) & 1ull)) continue;
            double x[D];
            for (int c = 0; c < D; ++c) x[c] = A[((size_t)p * m_max + r) * D + c];
            double bb = b[(size_t)p * m_max + r];
            if (!plp::fm::stage<D>(x, bb, shift, passes)) continue;
            const int cls = ELIM ? plp::fm::classify(plp::fm::pick<D>(x, col), tol) : (int)plp::fm::CLS_N;
            for (int c = 0; c < D; ++c) rows[nv * (D + 1) + c] = x[c];
            rows[nv * (D + 1) + D] = bb;
            if (cls == plp::fm::CLS_P) lP[nP++] = nv;
            if (cls == plp::fm::CLS_Q) lQ[nQ++] = nv;
            if (cls == plp::fm::CLS_N) lN[nN++] = nv;
            ++nv;
        }
        const long long npq = (long long)nP * nQ, cnt = npq + nN;
        if (count) count[p] = (int)cnt;
        if (!mout) continue;
        if (cnt > mo_max) { mout[p] = -1; continue; }
        int out_n = 0;
        for (long long t = 0; t < cnt; ++t) {
            double y[DO > 0 ? DO : 1];
            double yb = 0.0;
            bool ok;
            constexpr int S = D + 1;
            if constexpr (ELIM) {
                if (t < npq) {
                    const int j = lP[t / nQ], k = lQ[t % nQ];
                    ok = plp::fm::combine<D>(rows + j * S, rows[j * S + D], rows + k * S, rows[k * S + D], col, y, yb);
                } else {
                    const int j = lN[t - npq];
                    ok = plp::fm::pass_through<D>(rows + j * S, rows[j * S + D], col, y, yb);
                }
            } else {
                const int j = lN[t];
                for (int c = 0; c < D; ++c) y[c] = rows[j * S + c];
                yb = rows[j * S + D];
                ok = true;
            }
            if (!ok) continue;
            for (int c = 0; c < DO; ++c) Aout[((size_t)p * mo_max + out_n) * DO + c] = y[c];
            bout[(size_t)p * mo_max + out_n] = yb;
            ++out_n;
        }
        for (int r = out_n; r < mo_max; ++r) {
            for (int c = 0; c < DO; ++c) Aout[((size_t)p * mo_max + r) * DO + c] = 0.0;
            bout[(size_t)p * mo_max + r] = 0.0;
        }
        mout[p] = out_n;
    }
}

template <int D>
int dispatch(long long B, int m_max, const double* A, const double* b, const int* m, const uint64_t* keep, int kw,
             const int* flags, int col, int first, double tol, int mo_max, int* count, double* Aout, double* bout,
             int* mout) {
    if (col >= 0) {
        if constexpr (D >= 2) {
            step<D, true>(B, m_max, A, b, m, keep, kw, flags, col, first, tol, mo_max, count, Aout, bout, mout);
            return 0;
        }
        return 2;
    }
    step<D, false>(B, m_max, A, b, m, keep, kw, flags, col, first, tol, mo_max, count, Aout, bout, mout);
    return 0;
}

}  // namespace

extern "C" int fm_step(long long B, int m_max, int d, const double* A, const double* b, const int* m, const uint64_t* keep,
                       int kw, const int* flags, int col, int first, double tol, int mo_max, int* count, double* Aout,
                       double* bout, int* mout) {
    if (m_max > 4096) return 2;
#define FM_D(DD) \
    case DD: return dispatch<DD>(B, m_max, A, b, m, keep, kw, flags, col, first, tol, mo_max, count, Aout, bout, mout);
    switch (d) {
        FM_D(1) FM_D(2) FM_D(3) FM_D(4) FM_D(5) FM_D(6) FM_D(7) FM_D(8) FM_D(9) FM_D(10) FM_D(11) FM_D(12) FM_D(13)
        FM_D(14) FM_D(15) FM_D(16)
        default: return 2;
    }
#undef FM_D
}
