// Host build of polytope_amd/csrc/plp_rdiff_search.hpp (the search of region_diff without its device backend): TEST
// INFRASTRUCTURE, compiled with g++ -ffp-contract=off by tests/rdiff_host.py.  The backend here forwards every sub-batch
// to a C callback, so the caller decides what the radius of a row list is and sees exactly which lists are asked.
//
// -DRDIFF_HOST_MAIN adds a main(): a stand-alone program that searches axis-aligned tables it makes itself (a box minus
// boxes, d = 2 and 3, the radius of a row list in closed form) with default knobs, without speculation and with a small
// backend and memo, after single moves on hand-made states (an empty list of indices, indices that wrap), for a run under -fsanitize=address,undefined without anything loaded into an interpreter.
#include <stdint.h>

#include <vector>

#include "../../polytope_amd/csrc/plp_rdiff_search.hpp"

// list k = rows[off[k] .. off[k + 1]) (off[0] need not be 0) -> radii_out[k]; 0, or a positive code that ends the search
typedef int (*rdiff_radii_fn)(long long n, const int32_t* off, const int32_t* rows, double* radii_out, void* user);

namespace {

struct CallbackBackend {
    rdiff_radii_fn fn;
    void* user;
    size_t lp, nrows;
    std::vector<double> out;
    size_t cap_lp() const { return lp; }
    size_t cap_rows() const { return nrows; }
    int solve(const int32_t* off, const int32_t* rows, size_t n, const double** radii, size_t* stride) {
        out.assign(n, 0.0);
        *radii = out.data();
        *stride = 1;
        return fn((long long)n, off, rows, out.data(), user);
    }
};

}  // namespace

// knobs[5] = sib, chain_scan, chain_node, deep, child (NULL: the defaults); cap_lp / cap_rows / memo_limit <= 0: what
// the library uses.  Leaves go to kind[max_leaves], off[max_leaves + 1], rows[max_rows]; counts[5] = leaves, rows,
// n_requests, n_scan_miss, n_node_miss.  Returns the search's code (plp::rdiff::Err, or the callback's), or -100 when
// the leaves do not fit the buffers (counts[0..1] say what is needed).
extern "C" int rdiff_search_host(int m, int N, const int32_t* mi, double abs_tol, const int32_t* knobs, long long cap_lp,
                                 long long cap_rows, long long memo_limit, rdiff_radii_fn fn, void* user,
                                 long long max_leaves, long long max_rows, int32_t* kind, int32_t* off, int32_t* rows,
                                 long long* counts) {
    plp::rdiff::Spec spec;
    if (knobs) { spec.sib = knobs[0]; spec.chain_scan = knobs[1]; spec.chain_node = knobs[2]; spec.deep = knobs[3]; spec.child = knobs[4]; }
    CallbackBackend be{fn, user, cap_lp > 0 ? (size_t)cap_lp : (size_t)1 << 15, cap_rows > 0 ? (size_t)cap_rows : (size_t)1 << 21, {}};
    plp::rdiff::Result res;
    plp::rdiff::Search<CallbackBackend> search(m, N, mi, abs_tol, spec, be, res, memo_limit > 0 ? (size_t)memo_limit : (size_t)1 << 20);
    const int rc = search.run();
    counts[0] = (long long)res.kind.size();
    counts[1] = (long long)res.rows.size();
    counts[2] = res.n_requests;
    counts[3] = res.n_scan_miss;
    counts[4] = res.n_node_miss;
    if (counts[0] > max_leaves || counts[1] > max_rows) return -100;
    for (size_t k = 0; k < res.kind.size(); ++k) kind[k] = res.kind[k];
    for (size_t k = 0; k < res.off.size(); ++k) off[k] = res.off[k];
    for (size_t k = 0; k < res.rows.size(); ++k) rows[k] = res.rows[k];
    return rc;
}

// One move on a hand-made state: counter[N], idx[n_idx] and level are loaded into a plp::rdiff::State (states no whole
// search reaches included), move 0 = next_sibling, 1 = reopen_after_piece, then resolve.  counter / level are updated
// in place; idx_out[idx_cap] / rows_out[idx_cap] get the INDICES and their table rows.  out[4] = ended, resolve ok,
// length of idx, sum of the counters as the State keeps it.  Returns 0, or -100 when idx_cap is too small.
extern "C" int rdiff_move_host(int m, int N, const int32_t* mi, int32_t* counter, long long n_idx, const long long* idx,
                               long long* level, int move, long long idx_cap, long long* idx_out, int32_t* rows_out,
                               long long* out) {
    const plp::rdiff::Table t(m, N, mi);
    plp::rdiff::State s(t);
    for (int j = 0; j < N; ++j) s.set_counter(j, counter[j]);
    s.idx.assign(idx, idx + n_idx);
    s.level = *level;
    const bool ended = move == 0 ? s.next_sibling() : s.reopen_after_piece();
    std::vector<int32_t> rows;
    const bool ok = s.resolve(rows);
    out[0] = ended;
    out[1] = ok;
    out[2] = (long long)s.idx.size();
    out[3] = s.sumc;
    *level = s.level;
    for (int j = 0; j < N; ++j) counter[j] = s.counter[j];
    if ((long long)s.idx.size() > idx_cap) return -100;
    for (size_t k = 0; k < s.idx.size(); ++k) idx_out[k] = s.idx[k];
    for (size_t k = 0; ok && k < rows.size(); ++k) rows_out[k] = rows[k];
    return 0;
}

#ifdef RDIFF_HOST_MAIN
#include <stdio.h>

namespace {

uint64_t g_s = 12345;
double unif() {   // a 64-bit LCG (Knuth's MMIX constants), [0, 1)
    g_s = g_s * 6364136223846793005ull + 1442695040888963407ull;
    return (double)(g_s >> 11) * (1.0 / 9007199254740992.0);
}

// row r of the table: sign * x[axis] <= bound
struct BoxTable {
    int d;
    std::vector<int> axis, sign;
    std::vector<double> bound;
    long long lists = 0;
};

// the Chebyshev radius of an axis-aligned row list: min over the axes of (smallest upper bound - largest lower bound) / 2,
// 0 where negative; NaN (no verdict) where an axis is not bounded on both sides
int box_radii(long long n, const int32_t* off, const int32_t* rows, double* out, void* user) {
    BoxTable& T = *static_cast<BoxTable*>(user);
    for (long long k = 0; k < n; ++k) {
        double ub[3] = {1e300, 1e300, 1e300}, lb[3] = {-1e300, -1e300, -1e300}, r = 1e300;
        for (int32_t q = off[k]; q < off[k + 1]; ++q) {
            const int row = rows[q], a = T.axis[row];
            if (T.sign[row] > 0) ub[a] = T.bound[row] < ub[a] ? T.bound[row] : ub[a];
            else lb[a] = -T.bound[row] > lb[a] ? -T.bound[row] : lb[a];
        }
        for (int a = 0; a < T.d; ++a) {
            if (ub[a] == 1e300 || lb[a] == -1e300) { r = __builtin_nan(""); break; }
            const double w = 0.5 * (ub[a] - lb[a]);
            r = w < r ? w : r;
        }
        out[k] = r < 0.0 ? 0.0 : r;
        T.lists++;
    }
    return 0;
}

struct Run {
    int rc;
    std::vector<int32_t> kind, off, rows;
    long long counts[5];
    bool same_leaves(const Run& o) const {
        if (rc != o.rc) return false;
        if (rc != 0) return true;
        return counts[2] == o.counts[2] && kind == o.kind && off == o.off && rows == o.rows;
    }
};

Run search(BoxTable& T, int m, const std::vector<int32_t>& mi, const int32_t* knobs, long long cap_lp, long long cap_rows,
           long long memo_limit) {
    Run r;
    r.kind.resize(1 << 12);
    r.off.resize((1 << 12) + 1);
    r.rows.resize(1 << 18);
    r.rc = rdiff_search_host(m, (int)mi.size(), mi.data(), 1e-7, knobs, cap_lp, cap_rows, memo_limit, box_radii, &T, 1 << 12,
                             1 << 18, r.kind.data(), r.off.data(), r.rows.data(), r.counts);
    r.kind.resize(r.counts[0]);
    r.off.resize(r.counts[0] + 1);
    r.rows.resize(r.counts[1]);
    return r;
}

// one move on a hand-made state (MOVE_STATES of tests/test_rdiff_search_host.py) and what rdiff_move_host must report
struct MoveCase {
    int m;
    std::vector<int32_t> mi, counter;
    std::vector<long long> idx;
    long long level;
    int move;
    long long ended, resolved, n_idx, level_after;
};
const MoveCase MOVES[] = {
    // an empty list of indices under an open cell within mi: "- M" has no last index, resolve fails
    {0, {2}, {1}, {}, 0, 0, 0, 0, 1, 0},
    {0, {2, 1}, {1, 0}, {}, 1, 1, 0, 0, 1, 0},
    {2, {2}, {1}, {}, 0, 0, 0, 0, 1, 0},
    {1, {1, 2}, {0, 1}, {}, 0, 1, 0, 0, 1, -1},
    // ... under an exhausted cell: closed, nothing is read, the search ends
    {0, {1}, {2}, {}, 0, 0, 1, 1, 0, -1},
    // "- M" on a row of the minuend: the index wraps to the end of the table / leaves it
    {2, {2, 1}, {1, 0}, {0, 1}, 1, 1, 0, 1, 3, 0},
    {1, {3, 3}, {1, 1}, {-9}, 1, 1, 0, 0, 2, 0},
    {1, {3, 3}, {2, 0}, {0, -12}, 0, 0, 0, 0, 3, 0},
};
bool move_as_expected(const MoveCase& c) {
    std::vector<int32_t> counter = c.counter, rows(c.idx.size() + 2);
    std::vector<long long> idx_out(c.idx.size() + 2);
    long long level = c.level, out[4];
    const int rc = rdiff_move_host(c.m, (int)c.mi.size(), c.mi.data(), counter.data(), (long long)c.idx.size(), c.idx.data(),
                                   &level, c.move, (long long)idx_out.size(), idx_out.data(), rows.data(), out);
    return rc == 0 && out[0] == c.ended && out[1] == c.resolved && out[2] == c.n_idx && level == c.level_after;
}

}  // namespace

int main() {
    long long searches = 0, leaves = 0, bad = 0, ended[2] = {0, 0};
    for (const MoveCase& c : MOVES) bad += !move_as_expected(c);
    const int32_t none[5] = {0, 0, 0, 0, 0}, deep[5] = {600, 6, 8, 1, 1};
    for (int trial = 0; trial < 40; ++trial) {
        const int d = 2 + trial % 2, N = 1 + (int)(unif() * (d == 2 ? 7 : 5)), m = 2 * d;
        BoxTable T;
        T.d = d;
        std::vector<int32_t> mi(N, 2 * d);
        auto add_box = [&](const double* lo, const double* hi, double flip) {
            for (int a = 0; a < d; ++a) { T.axis.push_back(a); T.sign.push_back(flip > 0 ? 1 : -1); T.bound.push_back(flip * hi[a]); }
            for (int a = 0; a < d; ++a) { T.axis.push_back(a); T.sign.push_back(flip > 0 ? -1 : 1); T.bound.push_back(flip * -lo[a]); }
        };
        const double lo0[3] = {0, 0, 0}, hi0[3] = {1, 1, 1};
        add_box(lo0, hi0, 1.0);
        std::vector<double> lo(3 * N), hi(3 * N);
        for (int j = 0; j < N; ++j)
            for (int a = 0; a < d; ++a) {
                const double c = unif(), w = 0.05 + 0.3 * unif();
                lo[3 * j + a] = c - w;
                hi[3 * j + a] = c + w;
            }
        for (int j = 0; j < N; ++j) add_box(&lo[3 * j], &hi[3 * j], 1.0);
        for (int j = 0; j < N; ++j) add_box(&lo[3 * j], &hi[3 * j], -1.0);   // the negations of the cells' rows
        const Run a = search(T, m, mi, nullptr, 0, 0, 0);
        const Run b = search(T, m, mi, none, 0, 0, 0);
        const Run c = search(T, m, mi, deep, 0, 0, 0);
        const Run e = search(T, m, mi, nullptr, 5, 64, 600);   // sub-batches of 5 lists, a memo that is emptied often
        searches += 4;
        leaves += a.counts[0];
        ended[a.rc != 0]++;
        bad += !(a.rc == 0 || a.rc == plp::rdiff::BAD_INDEX) || !a.same_leaves(b) || !a.same_leaves(c) || !a.same_leaves(e);
    }
    printf("rdiff_search_host: %lld searches, %lld pieces, %lld tables ended with pieces, %lld with an index out of range, inconsistent: %lld\n",
           searches, leaves, ended[0], ended[1], bad);
    return bad ? 1 : 0;
}
#endif
