// plp_rdiff_batch.hpp -- region_diff_batch: many set differences in one launch, one whole search per wavefront
// (rdiff_batch_kernel, plp_rdiff_batch.hip).  This header is the sequential rule, compiled for the host (g++
// -ffp-contract=off, tests/cabi/rdiff_batch_host.cpp) and for the device, where ONE lane runs it on a State in LDS and the
// wavefront solves the Chebyshev LP it asks for:
//   the table build of region_diff (polytope.py:1726-1741, ref :2166-2183) on rows that are unit length already, and
//   the walk of plp_rdiff_walk.hpp (the table's shape, the moves, the verdicts of a scan and a node: the same code the
//   library search of plp_rdiff_search.hpp runs) on a State of fixed arrays, without memo or speculation: step() runs it
//   up to the next radius it has to read, returns, and is called again with that radius.
// It differs from the library search only in WHICH radii are read: a scan stops at its first hit, so a frame knows fewer
// dead cells than the library's (which solves every cell of a scan) and some LPs the library skips are issued.  The
// verdicts, and with them the pieces, are the same.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "plp_rdiff_walk.hpp"

namespace plp {
namespace rdb {

// the caps of one problem
constexpr int MAX_DIM = 4;       // d <= 4
constexpr int MAX_M = 64;        // rows of the minuend
constexpr int MAX_CELLS = 64;    // cells listed for one problem (the open cells are a 64-bit mask)
constexpr int MAX_TABLE = 256;   // m + 2M (a frame's row set is a 256-bit mask)
constexpr int MAX_LIST = 64;     // rows of any one list, a cell's rows included: one row per lane
constexpr int MAX_NEW = (MAX_TABLE - 1) / 2;        // M at m = 1
constexpr int MAX_STORED = MAX_TABLE / 2 + MAX_M / 2;   // m + M at m = 64: the negations are not stored
constexpr int IDX_CAP = MAX_LIST + 2;   // at most one row is pushed between two resolve()s
constexpr int MAX_FRAMES = 64;

enum Status : int {
    RD_OK = 0,
    RD_OVERFLOW = 1,      // more than p_max pieces or r_max rows: count / nrows say what is needed, what fits is written
    RD_COVERED = 2,       // a listed cell has no new row: the difference is empty
    RD_LONG = 3,          // a list of more than MAX_LIST rows
    RD_BUDGET = 4,        // max_lps LPs were not enough
    RD_INDEX = 5,         // resolve failed: the reference raises IndexError there
    RD_UNSUPPORTED = 6    // a cap on m / N / M / a cell's rows, or a cell index outside the table: nothing is run
};

enum : int { ACT_LP = 0, ACT_DONE = 1 };
enum : int { PH_TOP = 0, PH_SCAN_RESULT = 1, PH_SCAN_FINISH = 2, PH_NODE_REQUEST = 3, PH_NODE_RESULT = 4 };

// What an earlier scan decided: its rows, and the cells not SOLVED there with a radius <= abs_tol / 2
struct Frame {
    unsigned long long rows[MAX_TABLE / 64];
    unsigned long long alive;
};

// where the pieces go (kind[p_max], off[p_max + 1], rows[r_max] of ONE problem)
struct Out {
    int32_t *kind, *off, *rows;
    int p_max, r_max;
};

// Table and state of the walk in one
struct State {
    // ---- the table's shape: m rows of the minuend, M new rows (cell j from beg[j], mi[j] of them), their M negations
    int m, N, M, nrows;
    int mi[MAX_CELLS], beg[MAX_CELLS];
    // ---- the walk: counter, the reference's INDICES, the open cells as a mask
    int counter[MAX_CELLS];
    unsigned long long open;
    long long idx[IDX_CAP];
    int nidx;   // the length of INDICES (beyond IDX_CAP nothing is stored: the next resolve() ends the search, RD_LONG)
    long long level, sumc;
    int bad;    // a move read the last index of an empty list
    // ---- the search
    int cur[MAX_LIST], ncur;    // idx resolved to table rows
    int phase, scan_j;
    long long hit;
    double Rl;
    unsigned long long fr_alive, scan_todo;
    Frame frames[MAX_FRAMES];
    int nframes;
    // ---- the LP asked for: cur[0 .. ncur) and then the rows suf_beg .. suf_beg + suf_n - 1
    int suf_beg, suf_n;
    // ---- results
    int count, nout, nlp, status, over;
};

PLP_ENUM_FN unsigned long long cells_from(const int from) { return from >= 64 ? 0ull : ~0ull << from; }

// m, N, mi[] are set: the table's shape and the start of the walk.  (The caller has checked the caps.)
PLP_ENUM_FN void init(State& s) {
    for (int j = 0; j < s.N; ++j) s.counter[j] = 0;
    rdw::set_shape(s);
    s.open = 0ull;
    for (int i = 0; i < s.m; ++i) s.idx[i] = i;
    s.nidx = s.m;
    s.level = 0;
    s.sumc = 0;
    s.bad = 0;
    s.ncur = 0;
    s.phase = PH_TOP;
    s.scan_j = 0;
    s.hit = -1;
    s.Rl = 0.0;
    s.fr_alive = s.scan_todo = 0ull;
    s.nframes = 0;
    s.suf_beg = s.suf_n = 0;
    s.count = s.nout = s.nlp = s.over = 0;
    s.status = RD_OK;
}

// ---- the moves are those of plp_rdiff_walk.hpp; what they reach the table and the storage through
using rdw::set_counter, rdw::next_sibling, rdw::reopen_after_piece;
PLP_ENUM_FN const State& table_of(const State& s) { return s; }
PLP_ENUM_FN void last_minus(State& s, const long long M) {
    if (s.nidx < 1) s.bad = 1;
    else if (s.nidx <= IDX_CAP) s.idx[s.nidx - 1] -= M;
}
PLP_ENUM_FN void push(State& s, const long long v) {
    if (s.nidx < IDX_CAP) s.idx[s.nidx] = v;
    ++s.nidx;
}
PLP_ENUM_FN void keep_first(State& s, const long long n) {
    if ((long long)s.nidx > n) s.nidx = (int)n;
}
PLP_ENUM_FN int deepest_open(const State& s) { return 63 - __builtin_clzll(s.open); }
PLP_ENUM_FN int n_open(const State& s) { return __builtin_popcountll(s.open); }
// (whatever the bit was: setting it again costs less than a branch, 1 % of the 1 000-problem shape of 4.17)
PLP_ENUM_FN void mark_open(State& s, const int L, const bool, const bool on) {
    s.open = on ? s.open | 1ull << L : s.open & ~(1ull << L);
}
// idx -> cur.  RD_OK, RD_LONG, or RD_INDEX: an index is out of range, or a move found the list empty
PLP_ENUM_FN int resolve(State& s) {
    if (s.bad) return RD_INDEX;
    if (s.nidx > MAX_LIST) return RD_LONG;
    if (!rdw::rows_of(s, s.idx, s.nidx, s.cur)) return RD_INDEX;
    s.ncur = s.nidx;
    return RD_OK;
}

// cur is a piece.  Beyond p_max pieces or r_max rows the search goes on counting: nothing more is written, and the
// slots off[k + 1] of the pieces k < p_max that were not are set to -1
PLP_ENUM_FN void emit(State& s, const Out& o, const int kind) {
    if (!s.over && s.count < o.p_max && s.nout + s.ncur <= o.r_max) {
        o.kind[s.count] = kind;
        for (int k = 0; k < s.ncur; ++k) o.rows[s.nout + k] = s.cur[k];
        o.off[s.count + 1] = s.nout + s.ncur;
    } else {
        s.over = 1;
        if (s.count < o.p_max) o.off[s.count + 1] = -1;   // (a reader finds the pieces that were written without count)
    }
    s.count += 1;
    s.nout += s.ncur;
}

PLP_ENUM_FN int finish(State& s, const int status) {
    s.status = status != RD_OK ? status : (s.over ? RD_OVERFLOW : RD_OK);
    return ACT_DONE;
}
// the LP of cur + suf: counted against the budget
PLP_ENUM_FN int ask(State& s, const int max_lps, const int suf_beg, const int suf_n, const int next_phase) {
    if (s.ncur + suf_n > MAX_LIST) return finish(s, RD_LONG);
    if (s.nlp >= max_lps) return finish(s, RD_BUDGET);
    s.nlp += 1;
    s.suf_beg = suf_beg;
    s.suf_n = suf_n;
    s.phase = next_phase;
    return ACT_LP;
}
PLP_ENUM_FN int ask_scan_cell(State& s, const int max_lps) {
    s.scan_j = __builtin_ctzll(s.scan_todo);
    return ask(s, max_lps, s.beg[s.scan_j], s.mi[s.scan_j], PH_SCAN_RESULT);
}

// The walk up to the next radius it reads.  ACT_LP: solve cur[0 .. ncur) + rows suf_beg .. suf_beg + suf_n - 1 and call
// again with the radius as cheby_ball reads it (NaN: no verdict); ACT_DONE: s.status / count / nout / nlp are final.
// `R` is not looked at on the first call.  Every call ends after at most N moves: it asks for an LP, which the budget
// counts, or the search is over.
PLP_ENUM_FN int step(State& s, const Out& o, const double tol, const int max_lps, const double R) {
    for (;;) {
        switch (s.phase) {
            case PH_TOP: {
                if (s.level == -1) return finish(s, RD_OK);
                if (s.N == 0) {   // nothing to subtract: the minuend is the one piece
                    const int rc0 = resolve(s);
                    if (rc0) return finish(s, rc0);
                    emit(s, o, 0);
                    return finish(s, RD_OK);
                }
                if (s.counter[rdw::at(s, s.level)] != 0) {
                    if (next_sibling(s)) return finish(s, RD_OK);
                    s.phase = PH_NODE_REQUEST;
                    break;
                }
                // ---- scan: first cell j >= level whose stack with the current rows is full-dimensional
                const int rc = resolve(s);
                if (rc) return finish(s, rc);
                unsigned long long have[MAX_TABLE / 64] = {0ull, 0ull, 0ull, 0ull};
                for (int k = 0; k < s.ncur; ++k) {
                    const int r = s.cur[k];
                    const unsigned long long bit = 1ull << (r & 63);
                    // (a select per word instead of have[r >> 6]: a local array indexed at run time would live in scratch)
                    have[0] |= (r >> 6) == 0 ? bit : 0ull;
                    have[1] |= (r >> 6) == 1 ? bit : 0ull;
                    have[2] |= (r >> 6) == 2 ? bit : 0ull;
                    have[3] |= (r >> 6) == 3 ? bit : 0ull;
                }
                while (s.nframes > 0) {   // the top frame holds only while the current rows contain all of its rows
                    const Frame& f = s.frames[s.nframes - 1];
                    if (!((f.rows[0] & ~have[0]) | (f.rows[1] & ~have[1]) | (f.rows[2] & ~have[2]) | (f.rows[3] & ~have[3]))) break;
                    s.nframes -= 1;
                }
                const unsigned long long all = s.N >= 64 ? ~0ull : (1ull << s.N) - 1ull;
                s.fr_alive = s.nframes > 0 ? s.frames[s.nframes - 1].alive : all;
                s.scan_todo = s.fr_alive & all & cells_from((int)s.level);
                s.hit = -1;
                s.Rl = 0.0;
                if (s.nframes < MAX_FRAMES) {   // the frame this scan leaves (its `alive` is written when the scan ends)
                    Frame& f = s.frames[s.nframes];
                    f.rows[0] = have[0];
                    f.rows[1] = have[1];
                    f.rows[2] = have[2];
                    f.rows[3] = have[3];
                }
                if (!s.scan_todo) {
                    s.phase = PH_SCAN_FINISH;
                    break;
                }
                return ask_scan_cell(s, max_lps);
            }
            case PH_SCAN_RESULT: {
                const int j = s.scan_j;
                if (rdw::scan_dead(R, tol)) s.fr_alive &= ~(1ull << j);
                rdw::scan_read(R, tol, j, s.N, s.hit, s.Rl);
                s.scan_todo &= cells_from(j + 1);
                if (s.hit < 0 && s.scan_todo) return ask_scan_cell(s, max_lps);
                s.phase = PH_SCAN_FINISH;
                break;
            }
            case PH_SCAN_FINISH: {
                if (s.nframes < MAX_FRAMES) {   // (a full stack stops pushing: fewer cells are known dead)
                    s.frames[s.nframes].alive = s.fr_alive;
                    s.nframes += 1;
                }
                if (s.hit >= 0) {
                    s.level = s.hit;
                    set_counter(s, (int)s.hit, 1);
                    push(s, (long long)s.beg[s.hit] + s.M);
                }
                if (rdw::scan_emits(s.Rl, tol)) {
                    emit(s, o, 0);
                    if (reopen_after_piece(s)) return finish(s, RD_OK);
                }
                s.phase = PH_NODE_REQUEST;
                break;
            }
            case PH_NODE_REQUEST: {
                const int rc = resolve(s);
                if (rc) return finish(s, rc);
                return ask(s, max_lps, 0, 0, PH_NODE_RESULT);
            }
            default: {   // PH_NODE_RESULT: a piece when the node is full-dimensional at the last cell, else one level down
                if (rdw::node_full(R, tol)) {
                    if (s.level == s.N - 1) emit(s, o, 1);
                    else s.level = s.level + 1;
                }
                s.phase = PH_TOP;
                break;
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------------- the table build
// Is the cell row c (a[0 .. D), b at c[D]) a new row: sum_k |c[k] - p[k]| >= abs_tol for every minuend row p of T[m][D + 1],
// the terms added in index order (numpy's np.sum over a short last axis)
template <int D>
PLP_ENUM_FN bool row_is_new(const double (&c)[D + 1], const double* T, const int m, const double abs_tol) {
    bool is_new = true;
    for (int p = 0; p < m; ++p) {
        double sum = fabs(c[0] - T[p * (D + 1)]);
#pragma unroll
        for (int k = 1; k <= D; ++k) sum = sum + fabs(c[k] - T[p * (D + 1) + k]);
        is_new = is_new && (sum >= abs_tol);
    }
    return is_new;
}

// the caps that are known before any row is read; RD_OK or RD_UNSUPPORTED
PLP_ENUM_FN int check_shape(const int m, const int N) {
    return (m < 0 || m > MAX_M || N < 0 || N > MAX_CELLS) ? RD_UNSUPPORTED : RD_OK;
}
// ... and while cell after cell is added: M new rows so far, cnt more from a cell of mcj rows
PLP_ENUM_FN bool cell_fits(const int m, const int M, const int cnt, const int mcj) {
    return mcj <= MAX_LIST && m + 2 * (M + cnt) <= MAX_TABLE;
}

// row r of the m + 2M table from the m + M stored rows: the negations are formed on reading
PLP_ENUM_FN double table_at(const double* T, const int D1, const int m, const int M, const int r, const int k) {
    return r >= m + M ? -T[(r - M) * D1 + k] : T[r * D1 + k];
}

#if !defined(__HIPCC__)
// The sequential build: T[MAX_STORED][D + 1] gets the minuend's rows A[m][D], b[m] and then the new rows of the cells
// cell_idx[0 .. N) of the packed table CA[Nc][mc_max][D], Cb, mc, in cell order; s.m / s.N / s.mi are set, mi_out[N] and
// src_out[min(M, M_cap)] (global cell-row id c * mc_max + r of every new row) written.  RD_OK, RD_COVERED or RD_UNSUPPORTED
template <int D>
static inline int build_table(State& s, double* T, const int m, const double* A, const double* b, const long long Nc,
                              const int mc_max, const double* CA, const double* Cb, const int32_t* mc, const int N,
                              const int32_t* cell_idx, const double abs_tol, int32_t* mi_out, int32_t* src_out,
                              const int M_cap) {
    if (check_shape(m, N)) return RD_UNSUPPORTED;
    for (int j = 0; j < N; ++j)
        if (cell_idx[j] < 0 || cell_idx[j] >= Nc) return RD_UNSUPPORTED;
    for (int i = 0; i < m; ++i) {
        for (int k = 0; k < D; ++k) T[i * (D + 1) + k] = A[i * D + k];
        T[i * (D + 1) + D] = b[i];
    }
    s.m = m;
    s.N = N;
    int M = 0;
    bool covered = false;
    for (int j = 0; j < N; ++j) {
        const long long c = cell_idx[j];
        int mcj = mc ? mc[c] : mc_max;
        mcj = mcj < 0 ? 0 : (mcj > mc_max ? mc_max : mcj);
        if (mcj > MAX_LIST) return RD_UNSUPPORTED;
        int cnt = 0;
        for (int r = 0; r < mcj; ++r) {
            double row[D + 1];
            for (int k = 0; k < D; ++k) row[k] = CA[(c * mc_max + r) * D + k];
            row[D] = Cb[c * mc_max + r];
            if (!row_is_new<D>(row, T, m, abs_tol)) continue;
            if (!cell_fits(m, M, cnt + 1, mcj)) return RD_UNSUPPORTED;
            for (int k = 0; k <= D; ++k) T[(m + M + cnt) * (D + 1) + k] = row[k];
            if (M + cnt < M_cap) src_out[M + cnt] = (int32_t)(c * mc_max + r);
            ++cnt;
        }
        s.mi[j] = cnt;
        mi_out[j] = cnt;
        covered = covered || cnt == 0;
        M += cnt;
    }
    init(s);
    return covered ? RD_COVERED : RD_OK;
}
#endif

}  // namespace rdb
}  // namespace plp
