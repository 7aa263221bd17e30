// plp_rdiff_walk.hpp -- the walk of region_diff (ref :2201-2281), the counter / INDICES arithmetic of the reference with
// its odd turns ("level - 1" reading the LAST cell through Python's negative index, "- M" wrapping an index to the end of
// the table, rows trimmed to m + sum(counter)): the table's shape, the moves and the two verdict rules, once, for the
// library search (plp_rdiff_search.hpp: host, std::vector) and the batch kernel's rule (plp_rdiff_batch.hpp: host and
// device, fixed arrays in LDS).  Compiles for host and device (the pattern of plp_enum.hpp); no allocation, no error text.
//
// A table T has m, N, mi[], beg[], M, nrows.  A state S has counter[], level, sumc and keeps INDICES and the open cells in
// storage of its own, reached only through (found by argument-dependent lookup, next to S):
//   table_of(S&)          the table the state walks (a state may be its own)
//   last_minus(S&, M)     the last index minus M; S notes an empty list, and its resolve fails from then on (the
//                         reference raises IndexError there)
//   push(S&, v)           append an index
//   keep_first(S&, n)     drop the indices beyond the first n
//   deepest_open(S&)      the highest cell with counter != 0
//   n_open(S&)            how many cells have counter != 0
//   mark_open(S&, L, was, on)
//                         cell L's counter was / is now non-zero (called whenever a counter is set)
#pragma once
#include "plp_enum.hpp"

namespace plp {
namespace rdw {

// ---- the table's shape: m rows of the minuend, M = sum(mi) new rows of the N cells (cell j from beg[j]), their M negations
// t.m, t.N, t.mi[] are set -> t.beg[], t.M, t.nrows
template <class T>
PLP_ENUM_FN void set_shape(T& t) {
    decltype(t.M) M = 0;   // (a local: the table may live in LDS)
    for (int j = 0; j < t.N; ++j) {
        t.beg[j] = t.m + M;
        M += t.mi[j];
    }
    t.M = M;
    t.nrows = t.m + 2 * M;
}
// Python's negative indexing of counter / mi / beg (level == -1 reads the LAST cell, ref :2231)
template <class T>
PLP_ENUM_FN int at(const T& t, const long long level) { return (int)(level < 0 ? level + t.N : level); }
// the indices idx[0 .. n) as table rows, with Python's wrap of one that went below zero after "- M" (ref :2233); false:
// one is out of range (the reference raises IndexError there) and `rows` is not to be used
template <class T, class Row>
PLP_ENUM_FN bool rows_of(const T& t, const long long* idx, const int n, Row* rows) {
    for (int k = 0; k < n; ++k) {
        const long long r = idx[k] < 0 ? idx[k] + t.nrows : idx[k];
        if (r < 0 || r >= t.nrows) return false;
        rows[k] = (Row)r;
    }
    return true;
}

// ---- the moves.  counter[L]: 0 = cell closed; c = its first c - 1 new rows kept, row c negated; sumc = their sum
template <class S>
PLP_ENUM_FN void set_counter(S& s, const int L, const int v) {
    mark_open(s, L, s.counter[L] != 0, v != 0);
    s.sumc += v - s.counter[L];
    s.counter[L] = v;
}
// close cell L and drop the rows beyond the m + sumc the reference keeps
template <class S>
PLP_ENUM_FN void close_cell(S& s, const int L) {
    set_counter(s, L, 0);
    const long long keep_n = table_of(s).m + s.sumc;
    keep_first(s, keep_n < 0 ? 0 : keep_n);
}
// next sibling of the deepest open cell, closing exhausted cells on the way (ref :2246-2271); true: the search ends
template <class S>
PLP_ENUM_FN bool next_sibling(S& s) {
    const auto& t = table_of(s);
    while (n_open(s)) {   // deepest open cell first (the reference walks nzcount backwards)
        const int L = deepest_open(s);
        s.level = L;
        set_counter(s, L, s.counter[L] + 1);
        if (s.counter[L] <= t.mi[L]) {
            last_minus(s, t.M);
            push(s, (long long)t.beg[L] + s.counter[L] + t.M - 1);
            return false;
        }
        close_cell(s, L);
        s.level = s.level - 1;
        if (s.level == -1) return true;
    }
    return false;
}
// the move after a piece was emitted (ref :2230-2245: "level - 1", then re-open the cell there); true: the search ends
template <class S>
PLP_ENUM_FN bool reopen_after_piece(S& s) {
    const auto& t = table_of(s);
    s.level = s.level - 1;
    const int nz = n_open(s);
    for (int k = 0; k < nz; ++k) {
        const int L = at(t, s.level);
        if (s.counter[L] <= t.mi[L]) {
            last_minus(s, t.M);
            push(s, (long long)t.beg[L] + s.counter[L] + t.M);
            return false;
        }
        close_cell(s, L);
        if (s.level == -1) return true;
    }
    return false;
}

// ---- the verdicts.  R is a Chebyshev radius as cheby_ball reads it; NaN = the LP ended without a verdict (unbounded ball,
// iteration limit): the reference reads radius 0 there (ref :1294-1297) and solves the cell again at every node below.
//
// A scan reads the cells in ascending order up to its first hit.  The cell is dead below this node: only one whose LP was
// SOLVED with a radius <= tol / 2 is (NaN compares false)
PLP_ENUM_FN bool scan_dead(const double R, const double tol) { return R <= 0.5 * tol; }
// the radius of cell j, no cell before it having hit: a hit needs R > tol; Rl is the reference's R after its loop -- the
// hit's radius, else that of cell N - 1 if it was read, else the 0 it started as
PLP_ENUM_FN void scan_read(const double R, const double tol, const int j, const int N, long long& hit, double& Rl) {
    const double Rj = R != R ? 0.0 : R;
    if (Rj > tol) hit = j;
    if (Rj > tol || j == N - 1) Rl = Rj;
}
// after the scan: nothing left to subtract, the current rows are a piece (ref :2226-2245)
PLP_ENUM_FN bool scan_emits(const double Rl, const double tol) { return Rl < tol; }
// the node is full-dimensional: a piece at the last cell, else one level down
PLP_ENUM_FN bool node_full(const double R, const double tol) { return (R != R ? 0.0 : R) > tol; }

}  // namespace rdw
}  // namespace plp
