// plp_rdiff_search.hpp -- the search of region_diff (ref :2201-2281) over row lists of one constraint table, host only
// (no HIP, no error string, no environment): the twin of polytope._DiffSearch.  The walk -- the table's shape, the moves
// next_sibling / reopen_after_piece, the verdicts of a scan and a node -- is plp_rdiff_walk.hpp, run here on a State of
// std::vectors; this header adds a radius memo keyed by a hash of the row list, speculation on what the search asks
// next, and a queue solved in batches by a Backend: cap_lp() / cap_rows() = the most lists / rows of a sub-batch;
// solve(off, rows, n, &radii, &stride): list k = rows[off[k] .. off[k + 1]) -> its radius at radii[k * stride]; 0 or a
// code of its own.  plp_capi.hip runs it on plp_rdiff_host.hpp, tests/cabi/rdiff_search_host.cpp on a callback (CPU).
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <algorithm>
#include <chrono>
#include <numeric>
#include <vector>

#include "plp_rdiff_walk.hpp"

namespace plp {
namespace rdiff {

// what run() returns besides 0 and the backend's codes, which are positive: these stay negative.  The caller words them
enum Err : int { OK = 0, SCAN_MEMO = -1, RADIUS_MISSING = -2, BAD_INDEX = -3, LIST_TOO_LONG = -4 };

// 128-bit order-dependent hash of a row list, extendable by a suffix (lists are "current rows + a few more")
struct Key {
    uint64_t a, b;
    bool operator==(const Key& o) const { return a == o.a && b == o.b; }
};
inline Key key_push(Key k, int32_t r) {
    k.a = (k.a ^ (uint64_t)(uint32_t)(r + 1)) * 0x9E3779B97F4A7C15ull;
    k.a ^= k.a >> 29;
    k.b = (k.b + (uint64_t)(uint32_t)(r + 1)) * 0xC2B2AE3D27D4EB4Full;
    k.b ^= k.b >> 31;
    return k;
}
inline Key key_of_list(const int32_t* r, size_t n) {
    Key k{0x243F6A8885A308D3ull, 0x13198A2E03707344ull};
    for (size_t i = 0; i < n; ++i) k = key_push(k, r[i]);
    return k;
}

// open-addressing table Key -> radius; grows by rehashing, clear() touches only the occupied slots
struct RadiusTable {
    std::vector<Key> keys;
    std::vector<double> vals;
    std::vector<unsigned char> used;
    std::vector<uint32_t> slots;   // occupied positions, in insertion order
    size_t count = 0, mask = 0;
    void reset(size_t cap_pow2) {
        keys.assign(cap_pow2, Key{0, 0});
        vals.assign(cap_pow2, 0.0);
        used.assign(cap_pow2, 0);
        slots.clear();
        count = 0;
        mask = cap_pow2 - 1;
    }
    void clear() {
        for (uint32_t i : slots) used[i] = 0;
        slots.clear();
        count = 0;
    }
    const double* find(const Key& k) const {
        for (size_t i = (size_t)k.a & mask;; i = (i + 1) & mask) {
            if (!used[i]) return nullptr;
            if (keys[i] == k) return &vals[i];
        }
    }
    void put(const Key& k, double v) {
        if ((count + 1) * 2 > mask) grow();
        for (size_t i = (size_t)k.a & mask;; i = (i + 1) & mask) {
            if (!used[i]) { used[i] = 1; keys[i] = k; vals[i] = v; ++count; slots.push_back((uint32_t)i); return; }
            if (keys[i] == k) { vals[i] = v; return; }
        }
    }
    void grow() {
        std::vector<Key> ok;
        std::vector<double> ov;
        ok.reserve(count);
        ov.reserve(count);
        for (uint32_t i : slots) { ok.push_back(keys[i]); ov.push_back(vals[i]); }
        reset((mask + 1) * 2);
        for (size_t t = 0; t < ok.size(); ++t) put(ok[t], ov[t]);
    }
};

// The Chebyshev radii the search asks for, keyed by the row list, and the lists queued for the next batch.  A miss
// triggers ONE flush holding the missing list plus whatever the search will need next (speculation).
struct RadiusMemo {
    size_t limit;                 // entries beyond which the memo is emptied before a flush
    RadiusTable memo, pending;    // pending: key -> position in the batch being assembled
    std::vector<int32_t> prow, poff;
    std::vector<Key> pkey;
    double t_store = 0.0;         // seconds spent putting the radii of the batches into the memo
    int too_long = 0;             // LIST_TOO_LONG: the rows of the list no sub-batch holds
    explicit RadiusMemo(size_t limit_ = (size_t)1 << 20) : limit(limit_) {
        memo.reset(1 << 14);
        pending.reset(1 << 12);
        poff.assign(1, 0);
    }
    const double* find(const Key& k) const { return memo.find(k); }
    // queue the list base[0..nb) + suf[0..ns) (key given) for the next batch unless known or queued already; `required`:
    // the search cannot continue without this radius (only speculative lists are subject to the bound on one batch)
    void want(const Key& k, const int32_t* base, size_t nb, const int32_t* suf, size_t ns, bool required = false) {
        if (memo.find(k) || pending.find(k)) return;
        if (!required && pkey.size() >= (1u << 16)) return;
        pending.put(k, (double)pkey.size());
        pkey.push_back(k);
        prow.insert(prow.end(), base, base + nb);
        prow.insert(prow.end(), suf, suf + ns);
        poff.push_back((int32_t)prow.size());
    }
    // solve everything queued, in sub-batches cut by the backend's capacities; results go to the memo
    template <class Backend>
    int flush(Backend& be) {
        const size_t total = pkey.size(), cap_lp = be.cap_lp(), cap_rows = be.cap_rows();
        // radii are consumed soon after they are computed.  The memo is emptied only BEFORE the first sub-batch, never
        // between two of them, so everything this call stores is there when it returns (a caller that skipped a list
        // because it was known before the call asks again: see the retry loop of the scan)
        if (memo.count + total > limit) memo.clear();
        for (size_t done = 0; done < total;) {
            size_t n = 0, nr = 0;
            while (done + n < total && n < cap_lp && nr + (size_t)(poff[done + n + 1] - poff[done + n]) <= cap_rows) {
                nr += (size_t)(poff[done + n + 1] - poff[done + n]);
                ++n;
            }
            if (n == 0) { too_long = poff[done + 1] - poff[done]; return LIST_TOO_LONG; }
            const double* radii = nullptr;
            size_t stride = 1;
            int rc = be.solve(poff.data() + done, prow.data(), n, &radii, &stride);
            if (rc) return rc;
            const auto t0 = std::chrono::steady_clock::now();
            for (size_t k = 0; k < n; ++k) memo.put(pkey[done + k], radii[k * stride]);
            t_store += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
            done += n;
        }
        pkey.clear();
        prow.clear();
        poff.assign(1, 0);
        pending.clear();
        return OK;
    }
};

// the table's shape (plp_rdiff_walk.hpp), cells without a cap
struct Table {
    int m, N;
    const int32_t* mi;
    std::vector<long long> beg;
    long long M = 0, nrows = 0;
    Table(int m_, int N_, const int32_t* mi_) : m(m_), N(N_), mi(mi_), beg(N_) { rdw::set_shape(*this); }
};

// The state of the walk; a speculation runs the moves on a COPY to see which nodes follow, so the lists are exactly the
// ones the search will form (odd turns of the INDICES arithmetic included).
struct State {
    const Table* t;
    std::vector<int> counter;      // per cell; `sumc` = their sum
    std::vector<int> open_cells;   // cells with counter != 0, ascending
    std::vector<long long> idx;    // the reference's INDICES (may hold wrapped / out-of-range values)
    long long level = 0, sumc = 0;
    bool bad = false;              // a move read the last index of an empty list
    explicit State(const Table& tb) : t(&tb), counter(tb.N, 0), idx(tb.m) { std::iota(idx.begin(), idx.end(), 0LL); }
    // ---- the moves of plp_rdiff_walk.hpp on this state
    void set_counter(int L, int v) { rdw::set_counter(*this, L, v); }
    bool next_sibling() { return rdw::next_sibling(*this); }
    bool reopen_after_piece() { return rdw::reopen_after_piece(*this); }
    // ---- what they reach the table and the storage through
    friend const Table& table_of(const State& s) { return *s.t; }
    friend void last_minus(State& s, long long M) {
        if (s.idx.empty()) s.bad = true;
        else s.idx.back() -= M;
    }
    friend void push(State& s, long long v) { s.idx.push_back(v); }
    friend void keep_first(State& s, long long n) {
        if ((long long)s.idx.size() > n) s.idx.resize(n);
    }
    friend int deepest_open(const State& s) { return s.open_cells.back(); }
    friend int n_open(const State& s) { return (int)s.open_cells.size(); }
    friend void mark_open(State& s, int L, bool was, bool on) {
        if (was == on) return;
        const auto it = std::lower_bound(s.open_cells.begin(), s.open_cells.end(), L);
        if (on) s.open_cells.insert(it, L);
        else s.open_cells.erase(it);
    }
    // idx as table rows; false: an index is out of range or a move found the list empty (the reference raises IndexError
    // there) and `rows` is not to be used
    bool resolve(std::vector<int32_t>& rows) const {
        rows.resize(idx.size());
        return !bad && rdw::rows_of(*t, idx.data(), (int)idx.size(), rows.data());
    }
};

// How far the speculation goes: the bound on the lists of a cell's sibling chain, the steps of the
// empty chain queued with a scan / with a node, the first alive cell's child scan one level down, the first child of
// every alive cell with a scan
struct Spec { int sib = 100, chain_scan = 6, chain_node = 8, deep = 0, child = 1; };

// the pieces in order -- leaf k: kind[k] (0 = as is, ref :2229; 1 = to be reduce()d, ref :2276), rows[off[k] .. off[k + 1])
struct Result {
    std::vector<int32_t> kind, off = {0}, rows;
    long long n_requests = 0, n_scan_miss = 0, n_node_miss = 0;
};

// What earlier scans already decided.  A cell whose stack with the rows of an ANCESTOR node had radius <= abs_tol / 2
// cannot reach abs_tol with more rows added (the set only shrinks; LP values are exact to ~1e-12), so its LP is not
// issued again below that node: it counts as "no hit", which is what the reference would find.  A frame = the rows a
// scan was made with + the cells that stayed alive; it is used only while the current rows contain all of its rows
// (checked, because the reference's INDICES arithmetic does not always nest).
struct Frame { std::vector<int32_t> rows; std::vector<int> alive; };

template <class Backend>
class Search {
public:
    RadiusMemo R;
    double t_spec = 0.0;   // seconds spent assembling the lists of the batches

    Search(int m, int N, const int32_t* mi, double abs_tol, const Spec& spec, Backend& be, Result& res,
           size_t memo_limit = (size_t)1 << 20)
        : R(memo_limit), t(m, N, mi), tol(abs_tol), sp(spec), be(be), res(res), s(t), mult(t.nrows, 0), all_cells(N) {
        for (int j = 0; j < N; ++j) all_cells[j] = j;
    }

    int run() {
        while (s.level != -1) {
            bool ended = false;
            int rc = OK;
            if (s.counter[rdw::at(t, s.level)] == 0) rc = scan(ended);
            else ended = s.next_sibling();
            if (rc || ended) return rc;
            rc = node();
            if (rc) return rc;
        }
        return OK;
    }

private:
    using Clock = std::chrono::steady_clock;
    const Table t;
    const double tol;
    const Spec sp;
    Backend& be;
    Result& res;
    State s;
    std::vector<Frame> frames;
    std::vector<int> mult, all_cells;
    std::vector<int32_t> cur, suf, child, sim;   // cur = s.idx resolved to table rows

    // the key of cell j's scan list (the rows of `kbase` + ALL new rows of the cell)
    Key scan_key(Key k, int j) const {
        for (int r = 0; r < t.mi[j]; ++r) k = key_push(k, (int32_t)(t.beg[j] + r));
        return k;
    }
    void emit(int kind) {
        res.kind.push_back(kind);
        res.rows.insert(res.rows.end(), cur.begin(), cur.end());
        res.off.push_back((int32_t)res.rows.size());
    }
    const std::vector<int>& alive_now() {   // needs `cur` resolved
        for (int32_t r : cur) mult[r]++;
        while (!frames.empty()) {
            bool sub = true;
            for (int32_t r : frames.back().rows) if (!mult[r]) { sub = false; break; }
            if (sub) break;
            frames.pop_back();
        }
        for (int32_t r : cur) mult[r]--;
        return frames.empty() ? all_cells : frames.back().alive;
    }
    // queue, for every alive cell j >= from: the stack of `base` with ALL its new rows (the scan, ref :2212-2224) and
    // with its first new row negated (the node the search enters when j is the first hit).  `required`: the scan lists
    // are what the search is waiting for (queued first, exempt from the bound on a batch); the first children are
    // speculation
    void queue_scan1(const std::vector<int>& alive, long long from, const Key& kbase, const std::vector<int32_t>& base,
                     bool required) {
        for (int j : alive) {
            if (j < from) continue;
            suf.resize(t.mi[j]);
            for (int r = 0; r < t.mi[j]; ++r) suf[r] = (int32_t)(t.beg[j] + r);
            R.want(scan_key(kbase, j), base.data(), base.size(), suf.data(), suf.size(), required);
        }
        if (!sp.child) return;
        for (int j : alive) {
            if (j < from) continue;
            const int32_t neg = (int32_t)(t.beg[j] + t.M);
            R.want(key_push(kbase, neg), base.data(), base.size(), &neg, 1);
        }
    }
    // ... and, for the cell the scan will most likely stop at (the first one still alive): the same one level further
    // down (sp.deep: when that guess is right the search descends two levels on one batch), and its whole sibling
    // chain (rows 1..c-1 of the cell kept, row c negated) with the scans they need when they are not empty, as long
    // as that stays within sp.sib lists
    void queue_scan(const std::vector<int>& alive, long long from, const Key& kbase, bool required) {
        queue_scan1(alive, from, kbase, cur, required);
        auto first = std::lower_bound(alive.begin(), alive.end(), from);
        if (first == alive.end()) return;
        const int j = *first;
        if (j < t.N - 1 && sp.deep) {
            child = cur;
            child.push_back((int32_t)(t.beg[j] + t.M));
            queue_scan1(alive, (long long)j + 1, key_push(kbase, (int32_t)(t.beg[j] + t.M)), child, false);
        }
        const long long n_after = alive.end() - (first + 1);
        if ((long long)t.mi[j] * (2 * n_after + 1) > sp.sib) return;
        child = cur;
        Key kc = kbase;
        for (int c = 2; c <= t.mi[j]; ++c) {
            child.push_back((int32_t)(t.beg[j] + c - 2));
            kc = key_push(kc, (int32_t)(t.beg[j] + c - 2));
            const int32_t neg = (int32_t)(t.beg[j] + c - 1 + t.M);
            R.want(key_push(kc, neg), child.data(), child.size(), &neg, 1);
            if (j < t.N - 1) {
                child.push_back(neg);
                queue_scan1(alive, (long long)j + 1, key_push(kc, neg), child, false);
                child.pop_back();
            }
        }
    }
    // queue the node of state `c`; false: an index is out of range there
    bool want_state(const State& c) {
        if (!c.resolve(sim)) return false;
        R.want(key_of_list(sim.data(), sim.size()), sim.data(), sim.size(), nullptr, 0);
        return true;
    }
    // queue the nodes the search visits from state `c` on while every node turns out empty
    void queue_empty_chain(State& c, int steps) {
        for (int step = 0; step < steps; ++step) {
            if (c.level == -1 || c.counter[rdw::at(t, c.level)] == 0) break;   // the next move would be a scan (or the end)
            if (c.next_sibling()) break;
            if (!want_state(c)) break;
        }
    }
    bool scan_known(const std::vector<int>& alive, const Key& kbase) const {
        for (int j : alive)
            if (j >= s.level && !R.find(scan_key(kbase, j))) return false;
        return true;
    }
    // the radii of a scan, fetched and read -> the first cell that hits, the reference's R after its loop (the radius of
    // the LAST cell looked at), the frame the scan leaves (`alive` refers into `frames`: the caller pushes the frame)
    int scan_cells(Frame& fr, long long& hit, double& Rl) {
        if (!s.resolve(cur)) return BAD_INDEX;
        const Key kbase = key_of_list(cur.data(), cur.size());
        const std::vector<int>& alive = alive_now();
        for (int attempt = 0; !scan_known(alive, kbase); ++attempt) {   // (a full memo is emptied by flush(): ask again then)
            if (attempt == 3) return SCAN_MEMO;   // every attempt flushed: the memo cannot hold one scan
            res.n_scan_miss++;
            const auto ts0 = Clock::now();
            queue_scan(alive, s.level, kbase, true);
            State c = s;   // the outcome "no cell hits": a piece is emitted, then the node the search re-opens and what follows it
            if (!c.reopen_after_piece() && want_state(c)) queue_empty_chain(c, sp.chain_scan);
            t_spec += std::chrono::duration<double>(Clock::now() - ts0).count();
            const int rc = R.flush(be);
            if (rc) return rc;
        }
        fr.rows = cur;
        for (int j : alive) {
            if (j < s.level) continue;
            const double Rj = *R.find(scan_key(kbase, j));
            if (!rdw::scan_dead(Rj, tol)) fr.alive.push_back(j);
            if (hit < 0) {   // (the reference stops reading at the hit; the frame takes every cell)
                res.n_requests++;
                rdw::scan_read(Rj, tol, j, t.N, hit, Rl);
            }
        }
        return OK;
    }
    // ---- scan: first cell j >= level whose stack with the current rows is full-dimensional
    int scan(bool& ended) {
        Frame fr;
        long long hit = -1;
        double Rl = 0.0;
        const int rc = scan_cells(fr, hit, Rl);
        if (rc) return rc;
        frames.push_back(std::move(fr));
        if (hit >= 0) {
            s.level = hit;
            s.set_counter((int)hit, 1);
            push(s, t.beg[hit] + t.M);
        }
        if (rdw::scan_emits(Rl, tol)) {
            emit(0);
            ended = s.reopen_after_piece();
        }
        return OK;
    }
    // ---- the node itself: a piece when it is full-dimensional at the last cell, else one level down
    int node() {
        if (!s.resolve(cur)) return BAD_INDEX;
        const Key knode = key_of_list(cur.data(), cur.size());
        if (!R.find(knode)) {
            res.n_node_miss++;
            const auto ts0 = Clock::now();
            R.want(knode, cur.data(), cur.size(), nullptr, 0, true);
            State c = s;
            queue_empty_chain(c, sp.chain_node);
            // what it needs next when it is NOT empty: its scan and the first child of every cell still alive
            if (s.level >= 0 && s.level < t.N - 1) queue_scan(alive_now(), s.level + 1, knode, false);
            t_spec += std::chrono::duration<double>(Clock::now() - ts0).count();
            const int rc = R.flush(be);
            if (rc) return rc;
        }
        const double* pnode = R.find(knode);
        if (!pnode) return RADIUS_MISSING;
        res.n_requests++;
        if (rdw::node_full(*pnode, tol)) {
            if (s.level == t.N - 1) emit(1);
            else s.level = s.level + 1;
        }
        return OK;
    }
};

}  // namespace rdiff
}  // namespace plp
