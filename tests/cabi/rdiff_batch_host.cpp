// Host build of polytope_amd/csrc/plp_rdiff_batch.hpp (the sequential rule of rdiff_batch_kernel: table build, moves and
// search on fixed arrays): TEST INFRASTRUCTURE, compiled with g++ -ffp-contract=off by tests/rdiff_batch_host.py.  Every
// radius the rule reads is asked from a C callback, one list at a time, so the caller decides what the radius of a row list
// is and sees exactly which lists are asked, in order.
//
// -DRDIFF_BATCH_HOST_MAIN adds a main(): a stand-alone program that reads problems, the radius of every list their search
// asks and the leaves to expect from a text file (written by the test from its own run), and runs table build and search
// again, for a run under -fsanitize=address,undefined without anything loaded into an interpreter.
#include <stdint.h>
#include <string.h>

#include <vector>

#include "../../polytope_amd/csrc/plp_rdiff_batch.hpp"

namespace rdb = plp::rdb;

// list k = rows[off[k] .. off[k + 1]) -> radii_out[k] (n is always 1 here); 0, or a positive code that ends the search
typedef int (*rdiff_radii_fn)(long long n, const int32_t* off, const int32_t* rows, double* radii_out, void* user);

namespace {

// runs the search of a State that build_table() / init() left; out[4] = count, nrows, nlp, status.  0 or the callback's code
int run_search(rdb::State& s, double abs_tol, int max_lps, int p_max, int r_max, rdiff_radii_fn fn, void* user, int32_t* kind,
               int32_t* off, int32_t* rows, long long* out) {
    const rdb::Out o{kind, off, rows, p_max, r_max};
    off[0] = 0;
    double R = 0.0;
    int rc = 0;
    while (rdb::step(s, o, abs_tol, max_lps, R) == rdb::ACT_LP) {
        int32_t list[rdb::MAX_LIST];
        const int32_t loff[2] = {0, s.ncur + s.suf_n};
        for (int k = 0; k < s.ncur; ++k) list[k] = s.cur[k];
        for (int k = 0; k < s.suf_n; ++k) list[s.ncur + k] = s.suf_beg + k;
        rc = fn(1, loff, list, &R, user);
        if (rc) break;
    }
    out[0] = s.count;
    out[1] = s.nout;
    out[2] = s.nlp;
    out[3] = s.status;
    return rc;
}

template <int D>
int build_and_search(int m, const double* A, const double* b, long long Nc, int mc_max, const double* CA, const double* Cb,
                     const int32_t* mc, int N, const int32_t* cell_idx, double abs_tol, int max_lps, int p_max, int r_max,
                     rdiff_radii_fn fn, void* user, int32_t* kind, int32_t* off, int32_t* rows, long long* out, int32_t* mi,
                     int32_t* src, int M_cap, double* table) {
    rdb::State* s = new rdb::State();
    std::vector<double> T((size_t)rdb::MAX_STORED * (D + 1), 0.0);
    const int st = rdb::build_table<D>(*s, T.data(), m, A, b, Nc, mc_max, CA, Cb, mc, N, cell_idx, abs_tol, mi, src, M_cap);
    int rc = 0;
    off[0] = 0;
    out[0] = out[1] = out[2] = 0;
    out[3] = st;
    out[4] = 0;
    if (st != rdb::RD_UNSUPPORTED) {
        out[4] = s->M;
        // the whole m + 2M table as the search reads it (the negations are formed on reading)
        if (table)
            for (int r = 0; r < s->nrows; ++r)
                for (int k = 0; k <= D; ++k) table[r * (D + 1) + k] = rdb::table_at(T.data(), D + 1, s->m, s->M, r, k);
    }
    if (st == rdb::RD_OK) rc = run_search(*s, abs_tol, max_lps, p_max, r_max, fn, user, kind, off, rows, out);
    delete s;
    return rc;
}

}  // namespace

// One problem through table build and search.  A[m][d], b[m]; the cells cell_idx[0 .. N) of CA[Nc][mc_max][d], Cb, mc.
// Leaves go to kind[p_max], off[p_max + 1], rows[r_max]; out[5] = count, nrows, nlp, status, M; mi[N], src[M_cap];
// table[(m + 2M)][d + 1] (or NULL) gets the table.  Returns 0, the callback's code, or -1 for a d the rule is not built for.
extern "C" int rdiff_batch_host(int d, int m, const double* A, const double* b, long long Nc, int mc_max, const double* CA,
                                const double* Cb, const int32_t* mc, int N, const int32_t* cell_idx, double abs_tol,
                                int max_lps, int p_max, int r_max, rdiff_radii_fn fn, void* user, int32_t* kind, int32_t* off,
                                int32_t* rows, long long* out, int32_t* mi, int32_t* src, int M_cap, double* table) {
#define RDB_CASE(K)                                                                                                        \
    case K:                                                                                                                \
        return build_and_search<K>(m, A, b, Nc, mc_max, CA, Cb, mc, N, cell_idx, abs_tol, max_lps, p_max, r_max, fn, user, \
                                   kind, off, rows, out, mi, src, M_cap, table);
    switch (d) {
        RDB_CASE(1) RDB_CASE(2) RDB_CASE(3) RDB_CASE(4)
        default: return -1;
    }
#undef RDB_CASE
}

// The search alone on a table given by its shape (m, mi[N]): what plp::rdiff::Search runs in rdiff_search_host.
// out[4] = count, nrows, nlp, status (RD_UNSUPPORTED for a shape beyond the caps, RD_COVERED for an mi of 0).
extern "C" int rdiff_batch_search_host(int m, int N, const int32_t* mi, double abs_tol, int max_lps, int p_max, int r_max,
                                       rdiff_radii_fn fn, void* user, int32_t* kind, int32_t* off, int32_t* rows,
                                       long long* out) {
    off[0] = 0;
    out[0] = out[1] = out[2] = 0;
    out[3] = rdb::RD_UNSUPPORTED;
    if (rdb::check_shape(m, N)) return 0;
    int M = 0;
    bool covered = false;
    for (int j = 0; j < N; ++j) {
        if (mi[j] < 0 || !rdb::cell_fits(m, M, mi[j], mi[j])) return 0;
        covered = covered || mi[j] == 0;
        M += mi[j];
    }
    out[3] = rdb::RD_COVERED;
    if (covered) return 0;
    rdb::State* s = new rdb::State();
    s->m = m;
    s->N = N;
    for (int j = 0; j < N; ++j) s->mi[j] = mi[j];
    rdb::init(*s);
    const int rc = run_search(*s, abs_tol, max_lps, p_max, r_max, fn, user, kind, off, rows, out);
    delete s;
    return rc;
}

// One move on a hand-made state, as rdiff_move_host of rdiff_search_host.cpp (same arguments, same outputs) on the
// fixed-array State.  Returns 0, -100 when idx_cap is too small, -101 when the state does not fit the fixed arrays.
extern "C" int rdiff_batch_move_host(int m, int N, const int32_t* mi, int32_t* counter, long long n_idx, const long long* idx,
                                     long long* level, int move, long long idx_cap, long long* idx_out, int32_t* rows_out,
                                     long long* out) {
    if (rdb::check_shape(m, N) || N < 1 || n_idx > rdb::IDX_CAP - 1) return -101;
    rdb::State* s = new rdb::State();
    s->m = m;
    s->N = N;
    for (int j = 0; j < N; ++j) s->mi[j] = mi[j];
    rdb::init(*s);
    for (int j = 0; j < N; ++j) rdb::set_counter(*s, j, counter[j]);
    for (long long k = 0; k < n_idx; ++k) s->idx[k] = idx[k];
    s->nidx = (int)n_idx;
    s->level = *level;
    const bool ended = move == 0 ? rdb::next_sibling(*s) : rdb::reopen_after_piece(*s);
    const int rc = rdb::resolve(*s);
    out[0] = ended;
    out[1] = rc == rdb::RD_OK;
    out[2] = s->nidx;
    out[3] = s->sumc;
    *level = s->level;
    for (int j = 0; j < N; ++j) counter[j] = s->counter[j];
    int ret = 0;
    if (s->nidx > idx_cap || s->nidx > rdb::IDX_CAP) ret = -100;
    for (int k = 0; !ret && k < s->nidx; ++k) idx_out[k] = s->idx[k];
    for (int k = 0; !ret && rc == rdb::RD_OK && k < s->ncur; ++k) rows_out[k] = s->cur[k];
    delete s;
    return ret;
}

#ifdef RDIFF_BATCH_HOST_MAIN
#include <stdio.h>

#include <map>

namespace {

struct Replay {
    std::map<std::vector<int32_t>, double> radius;
    long long asked = 0, missing = 0;
};

int replay_radii(long long n, const int32_t* off, const int32_t* rows, double* out, void* user) {
    Replay& R = *static_cast<Replay*>(user);
    for (long long k = 0; k < n; ++k) {
        const std::vector<int32_t> key(rows + off[k], rows + off[k + 1]);
        const auto it = R.radius.find(key);
        R.asked++;
        if (it == R.radius.end()) {
            R.missing++;
            return 99;
        }
        out[k] = it->second;
    }
    return 0;
}

bool read_doubles(FILE* f, std::vector<double>& v, size_t n) {
    v.resize(n);
    for (size_t i = 0; i < n; ++i)
        if (fscanf(f, "%la", &v[i]) != 1) return false;
    return true;
}
bool read_ints(FILE* f, std::vector<int32_t>& v, size_t n) {
    v.resize(n);
    for (size_t i = 0; i < n; ++i)
        if (fscanf(f, "%d", &v[i]) != 1) return false;
    return true;
}

}  // namespace

// file: n_cases, then per case:  d m Nc mc_max N abs_tol(hex) max_lps p_max r_max / A / b / CA / Cb / mc / cell_idx /
// n_radii, then per radius: length, rows, radius (hex float or "nan") / count nrows status / kind[count] off[count + 1] rows
int main(int argc, char** argv) {
    if (argc < 2) return 2;
    FILE* f = fopen(argv[1], "r");
    if (!f) return 2;
    int n_cases = 0;
    if (fscanf(f, "%d", &n_cases) != 1) return 2;
    long long bad = 0, pieces = 0, lps = 0;
    for (int c = 0; c < n_cases; ++c) {
        int d, m, Nc, mc_max, N, max_lps, p_max, r_max, n_rad;
        double tol;
        if (fscanf(f, "%d %d %d %d %d %la %d %d %d", &d, &m, &Nc, &mc_max, &N, &tol, &max_lps, &p_max, &r_max) != 9) return 2;
        std::vector<double> A, b, CA, Cb;
        std::vector<int32_t> mc, cell_idx;
        if (!read_doubles(f, A, (size_t)m * d) || !read_doubles(f, b, m) || !read_doubles(f, CA, (size_t)Nc * mc_max * d) ||
            !read_doubles(f, Cb, (size_t)Nc * mc_max) || !read_ints(f, mc, Nc) || !read_ints(f, cell_idx, N))
            return 2;
        Replay R;
        if (fscanf(f, "%d", &n_rad) != 1) return 2;
        for (int k = 0; k < n_rad; ++k) {
            int len;
            if (fscanf(f, "%d", &len) != 1) return 2;
            std::vector<int32_t> key;
            std::vector<double> r;
            if (!read_ints(f, key, len) || !read_doubles(f, r, 1)) return 2;
            R.radius[key] = r[0];
        }
        int count, nrows, status;
        if (fscanf(f, "%d %d %d", &count, &nrows, &status) != 3) return 2;
        std::vector<int32_t> kind_w, off_w, rows_w;
        const int written = count < p_max ? count : p_max;
        if (!read_ints(f, kind_w, written) || !read_ints(f, off_w, written + 1) || !read_ints(f, rows_w, off_w[written])) return 2;
        // buffers of exactly the sizes the rule was told: a write past them is the sanitizer's to find
        std::vector<int32_t> kind(p_max), off(p_max + 1), rows(r_max), mi(N > 0 ? N : 1), src(rdb::MAX_NEW);
        long long out[5];
        const int rc = rdiff_batch_host(d, m, A.data(), b.data(), Nc, mc_max, CA.data(), Cb.data(), mc.data(), N,
                                        cell_idx.data(), tol, max_lps, p_max, r_max, replay_radii, &R, kind.data(), off.data(),
                                        rows.data(), out, mi.data(), src.data(), rdb::MAX_NEW, nullptr);
        bool ok = rc == 0 && out[0] == count && out[1] == nrows && out[3] == status && R.missing == 0;
        for (int k = 0; ok && k < written && off_w[k + 1] <= r_max; ++k) {
            ok = kind[k] == kind_w[k] && off[k + 1] == off_w[k + 1];
            for (int q = off_w[k]; ok && q < off_w[k + 1]; ++q) ok = rows[q] == rows_w[q];
        }
        bad += !ok;
        pieces += out[0];
        lps += out[2];
    }
    fclose(f);
    printf("rdiff_batch_host: %d problems, %lld pieces, %lld LPs, inconsistent: %lld\n", n_cases, pieces, lps, bad);
    return bad ? 1 : 0;
}
#endif
