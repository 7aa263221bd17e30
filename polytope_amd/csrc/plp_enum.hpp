// plp_enum.hpp -- what the enumeration kernels share: extreme_kernel (plp_extreme.*), hull_enum_kernel (plp_hull_enum.*) and
// volume_exact_kernel (plp_volume_exact.*) each put one member of the batch on one wavefront, stage its <= 64 live items
// compacted in LDS, and keep a host-compilable sequential rule that the kernel reproduces bit for bit ("the
// enumeration skeleton").  The first part also compiles for the host (g++ -ffp-contract=off, tests/cabi/*_host.cpp); the
// second (__HIPCC__) is its wave-level twin.  Tolerances, staging and outputs are the kernels' own, in their own headers.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define PLP_ENUM_FN __host__ __device__ __forceinline__
#else
#define PLP_ENUM_FN static inline
#endif

namespace plp {
namespace wenum {

constexpr int MAX_DIM = 4, MAX_ITEMS = 64;   // the dimensions the kernels are built for; one item (row, point) per lane

// f(dim<D>{}) for d = D in 1 .. MAX_DIM -> 0; non-zero for any other d (f is not called)
template <int D>
struct dim {
    static constexpr int value = D;
};
template <class F>
inline int dispatch_dim(const int d, F&& f) {
    switch (d) {
        case 1: f(dim<1>{}); return 0;
        case 2: f(dim<2>{}); return 0;
        case 3: f(dim<3>{}); return 0;
        case 4: f(dim<4>{}); return 0;
        default: return 2;
    }
}

// C(k, q) for q <= 3 and 0 <= k <= 64 (0 when k < q)
PLP_ENUM_FN int binom(const int k, const int q) {
    return q == 0 ? 1 : (q == 1 ? k : (q == 2 ? k * (k - 1) / 2 : k * (k - 1) * (k - 2) / 6));
}
// the number of candidates: C(n, D)
template <int D>
PLP_ENUM_FN int candidates(const int n) {
    return D == 4 ? (int)((long long)binom(n, 3) * (n - 3) / 4) : binom(n, D);
}

// the D-subset of {0 .. n - 1} of lexicographic rank r (0 <= r < C(n, D))
template <int D>
PLP_ENUM_FN void unrank(const int n, int r, int (&idx)[D]) {
    int c = 0;
#pragma unroll
    for (int pos = 0; pos < D; ++pos) {
        const int q = D - 1 - pos;   // items still to pick after this one
        if (q == 0) {
            c += r;
        } else {
            for (;;) {
                const int cnt = binom(n - 1 - c, q);
                if (r < cnt) break;
                r -= cnt;
                ++c;
            }
        }
        idx[pos] = c;
        ++c;
    }
}

// the subset after idx in lexicographic order; false when idx was the last
template <int D>
PLP_ENUM_FN bool next(const int n, int (&idx)[D]) {
    int pos = D - 1;
    while (pos >= 0 && idx[pos] == n - D + pos) --pos;
    if (pos < 0) return false;
    ++idx[pos];
    for (int k = pos + 1; k < D; ++k) idx[k] = idx[k - 1] + 1;
    return true;
}

// x.y, the products added in index order
template <int D>
PLP_ENUM_FN double dot(const double* x, const double* y) {
    double s = x[0] * y[0];
#pragma unroll
    for (int k = 1; k < D; ++k) s = s + x[k] * y[k];
    return s;
}

template <int D>
PLP_ENUM_FN double norm_inf(const double (&v)[D]) {
    double e = fabs(v[0]);
#pragma unroll
    for (int k = 1; k < D; ++k) e = fmax(e, fabs(v[k]));
    return e;
}

// one input row a x <= bi -> u = a / |a|_2 and nrm = |a|_2.  0: not staged (a zero row that says nothing), 1: staged,
// 2: the member is empty (a zero row with bi < 0 or NaN); u is set only for 1
template <int D>
PLP_ENUM_FN int unit_row(const double* a, const double bi, double (&u)[D], double& nrm) {
    nrm = sqrt(dot<D>(a, a));
    if (nrm == 0.0) return bi >= 0.0 ? 0 : 2;
#pragma unroll
    for (int k = 0; k < D; ++k) u[k] = a[k] / nrm;
    return 1;
}

// The sequential greedy list over the D-subsets of n items in lexicographic order (the twin of wave_greedy_round below).
//   candidate(idx) -> LIST_SKIP, LIST_TAKE (the caller now holds the candidate) or LIST_END (the list ends EMPTY: count = 0)
//   same(q)        -> the entry accepted at slot q is the held candidate to the caller's tolerance (the candidate's)
//   store(q, idx)     writes the held candidate to slot q
// A candidate is dropped when same(q) holds for some q < count, else it is stored at slot count.  -> overflow: a candidate
// distinct from the `cap` stored ones arrived; those stay, count = cap, the enumeration stops there.
enum : int { LIST_SKIP = 0, LIST_TAKE = 1, LIST_END = 2 };
template <int D, class Candidate, class Same, class Store>
PLP_ENUM_FN bool greedy_list(const int n, const int cap, int& count, Candidate&& candidate, Same&& same, Store&& store) {
    int idx[D];
    for (int k = 0; k < D; ++k) idx[k] = k;
    count = 0;
    do {
        const int kind = candidate(idx);
        if (kind == LIST_END) {
            count = 0;
            return false;
        }
        if (kind != LIST_TAKE) continue;
        bool dup = false;
        for (int q = 0; q < count && !dup; ++q) dup = same(q);
        if (dup) continue;
        if (count == cap) return true;
        store(count, idx);
        ++count;
    } while (next<D>(n, idx));
    return false;
}

#if defined(__HIPCC__)
// ------------------------------------------------------------------------------------------------ one member, one wavefront
constexpr int BLOCK = 64;   // one wavefront per workgroup

// min / max over the wavefront (every lane gets the result; exact, so the order of the butterfly does not matter)
__device__ __forceinline__ double wave_min(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmin(v, __shfl_xor(v, o));
    return v;
}
__device__ __forceinline__ double wave_max(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o));
    return v;
}

// The member prologue.  Workgroup P takes member P; lane i takes item i (at most 64: they are read from memory once), `live`
// when i < m (clamped to 0 .. m_max; m_max where `count` is null) and bit i of the keep word (all ones where `keepg` is null)
// is set.  The kernel stages its live item, then compact(): the lane writes its payload to LDS slot `pos`; the barrier follows.
struct Member {
    long long P;
    int lane, m;
    unsigned long long keep;
    bool live;
    unsigned long long staged;   // after compact(): the lanes whose item is staged,
    int n, pos;                  // how many they are, and how many of them stand before this lane

    __device__ __forceinline__ Member(const int m_max, const int* __restrict__ count,
                                      const unsigned long long* __restrict__ keepg)
        : P(blockIdx.x), lane(threadIdx.x) {
        m = count ? count[P] : m_max;
        m = m < 0 ? 0 : (m > m_max ? m_max : m);
        keep = keepg ? keepg[P] : ~0ull;
        live = lane < m && ((keep >> lane) & 1ull);
    }
    __device__ __forceinline__ void compact(const bool is_staged) {
        staged = __ballot(is_staged);
        n = __popcll(staged);
        pos = __popcll(staged & ((1ull << lane) - 1ull));
    }
};

// The greedy filter of one round of 64 candidates, lane `lane` holding one (ok: it is a candidate); cnt entries stand in the
// output, which this wavefront wrote in earlier rounds.  Every ok lane first compares with those (read back from global
// memory: a workgroup barrier stands between a round's stores and the next round's loads, and the arrays must not be
// __restrict__); the lanes that remain are resolved IN LANE ORDER -- the lowest one is accepted, stored and broadcast,
// the others drop out if they are close to it -- because closeness is not transitive and the sequential rule
// (greedy_list) compares a candidate with accepted entries only.  The tolerance is always the comparing lane's own.
//   same_stored(q) -> the entry at slot q is my candidate (every lane reads the same address)
//   same_lane(src) -> lane src's candidate, fetched with __shfl, is mine; called by ALL lanes of the wavefront
//   store(q)          writes my candidate to slot q
// -> overflow: a survivor arrived at cnt == cap (cnt stays cap, the rest of the round is not looked at).
template <class SameStored, class SameLane, class Store>
__device__ __forceinline__ bool wave_greedy_round(const int lane, bool ok, int& cnt, const int cap, SameStored&& same_stored,
                                                  SameLane&& same_lane, Store&& store) {
    if (!__any(ok)) return false;
    for (int q = 0; q < cnt; ++q) {   // the entries of earlier rounds
        const bool dup = same_stored(q);   // (not inside the &&: hipcc then packs the comparisons into bytes per entry,
        ok = ok && !dup;                   // measured 6 % slower on hull_enum_kernel<4> at 1 000 x (16, 4))
    }
    unsigned long long rem = __ballot(ok);
    const bool wrote = rem != 0ull;
    bool over = false;
    while (rem) {   // this round's survivors, in lane order
        if (cnt == cap) {
            over = true;
            break;
        }
        const int src = __ffsll((long long)rem) - 1;
        const bool dup = same_lane(src);
        if (lane == src) {
            store(cnt);
            ok = false;
        } else if (ok && dup) {
            ok = false;
        }
        ++cnt;
        rem = __ballot(ok);
    }
    if (wrote) __syncthreads();   // (uniform: the next round, and the end, read what this one stored)
    return over;
}

// the slots [from, to) of a list that ended early: NaN, and -1 in the index array where there is one
__device__ __forceinline__ void fill_tail(const int lane, double* x, int* index, const long long from, const long long to) {
    for (long long q = from + lane; q < to; q += BLOCK) {
        x[q] = __builtin_nan("");
        if (index) index[q] = -1;
    }
}
#endif   // __HIPCC__

}  // namespace wenum
}  // namespace plp
