// plp_envelope.hpp -- envelope_batch / is_convex_batch: the facet tests of envelope() (polytope.py envelope, ref :1414-1464) for
// many regions in one launch, one (region, member) list entry per wavefront (envelope_cross_kernel, plp_envelope.hip).
// This header is the rule, compiled for the host (g++ -ffp-contract=off, tests/cabi/envelope_host.cpp) and for the device,
// where every value of it is wave-uniform and the wavefront solves the Chebyshev LP behind radius().
//
// Input: a packed member table A[C][mc_max][d], b[C][mc_max], mc[C] (unit rows, as Polytope leaves them) and regions as
// index lists: region p lists the members mem_idx[reg_off[p] .. reg_off[p + 1]) (mem_idx NULL: entry w is member w).  Two
// regions, or two entries of one region, may list the same member.
// Work item: one list entry w -- member i = mem_idx[w] of region p, the owner of the facets under test.
//   for every OTHER entry j of the same list, in list order, and every row ii of i that is not yet crossed, in row order:
//       R = the Chebyshev radius of [rows of j; -a_ii x <= -b_ii], as cheby_ball reads it
//       row ii is crossed once some R > abs_tol
// The reference runs ii outer and j inner and never skips a test.  The verdict of a row is an OR over its tests, so the
// order of the loops and the skipping of rows that are crossed already change HOW MANY LPs run, never a verdict.
// No verdict: a test whose R is NaN, or abs_tol / 2 < R < 2 * abs_tol, says nothing -- it neither crosses the row nor clears
// it.  A row that ends not crossed with such a test behind it makes the entry ENV_OPEN; a row that another partner crosses
// clearly (R >= 2 * abs_tol) is simply crossed.  The single call decides r > abs_tol on the verified engines; the band keeps
// the two routes from differing by rounding at the threshold.  It is a condition, not a measurement.
// Output per entry: outer (bit ii set = row ii is outer), status, nlp.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "plp_enum.hpp"

namespace plp {
namespace env {

// the caps
constexpr int MAX_DIM = 8;     // d <= 8
constexpr int MAX_ROWS = 63;   // rows of a member: the stack [partner; one negated row] is one row per lane
constexpr int MAX_LIST = 64;   // rows of a stack (the MAX_LIST of plp_rdiff_batch.hpp)
// (no cap on the members of a region)

enum Status : int {
    ENV_OK = 0,
    ENV_OPEN = 1,          // a row is not crossed and one of its tests had no verdict: the single call decides
    ENV_UNSUPPORTED = 2    // a listed member with no row or more than MAX_ROWS, an index outside the table, or reg_off
                           // decreasing / outside mem_idx around this entry: nothing is run, outer = 0
};

// the state of one entry: wave-uniform on the device
struct Walk {
    unsigned long long rows;      // bit ii: row ii exists
    unsigned long long crossed;   // ... some partner reaches beyond it
    unsigned long long open;      // ... one of its tests had no verdict
    int nlp;
};

PLP_ENUM_FN unsigned long long rows_mask(const int mi) { return mi >= 64 ? ~0ull : (1ull << mi) - 1ull; }

// rows of member c as the rule reads them: mc[c] (NULL: mc_max), at most mc_max
PLP_ENUM_FN int member_rows(const int32_t* mc, const int mc_max, const long long c) {
    const int m = mc ? mc[c] : mc_max;
    return m > mc_max ? mc_max : m;
}
// may member c stand in a list
PLP_ENUM_FN bool member_ok(const long long c, const long long C, const int32_t* mc, const int mc_max) {
    if (c < 0 || c >= C) return false;
    const int m = member_rows(mc, mc_max, c);
    return m >= 1 && m <= MAX_ROWS;
}

// The region of entry w: the last p of 0 .. B - 1 with reg_off[p] <= w, by bisection; -1: none.  On a reg_off that
// decreases somewhere this is SOME p with reg_off[p] <= w; list_bounds() below refuses the entry unless that p's own two
// offsets hold it -- so an entry behind a decreasing step (w >= reg_off[p + 1]) is ENV_UNSUPPORTED, and whatever reg_off
// holds, no list is read that does not lie inside mem_idx[L].
PLP_ENUM_FN long long find_region(const int32_t* reg_off, const long long B, const long long w) {
    if (B < 1 || reg_off[0] > w) return -1;
    long long lo = 0, hi = B;   // reg_off[lo] <= w; hi = B or reg_off[hi] > w
    while (hi - lo > 1) {
        const long long mid = lo + (hi - lo) / 2;
        if (reg_off[mid] <= w) lo = mid;
        else hi = mid;
    }
    return lo;
}
// the list [lo, hi) of region p holds w and lies inside mem_idx[L]
PLP_ENUM_FN bool list_bounds(const int32_t* reg_off, const long long p, const long long w, const long long L, long long& lo,
                             long long& hi) {
    if (p < 0) return false;
    lo = reg_off[p];
    hi = reg_off[p + 1];
    return lo >= 0 && lo <= w && w < hi && hi <= L;
}

PLP_ENUM_FN void begin(Walk& s, const int mi) {
    s.rows = rows_mask(mi);
    s.crossed = s.open = 0ull;
    s.nlp = 0;
}
// the first row >= from that is still under test, or -1
PLP_ENUM_FN int next_row(const Walk& s, const int from) {
    const unsigned long long left = from >= 64 ? 0ull : (s.rows & ~s.crossed & (~0ull << from));
    return left ? __builtin_ctzll(left) : -1;
}
PLP_ENUM_FN bool no_verdict(const double R, const double tol) { return R != R || (R > 0.5 * tol && R < 2.0 * tol); }
// the radius of row ii's test against one partner
PLP_ENUM_FN void take(Walk& s, const int ii, const double R, const double tol) {
    s.nlp += 1;
    if (no_verdict(R, tol)) s.open |= 1ull << ii;
    else if (R > tol) s.crossed |= 1ull << ii;
}
PLP_ENUM_FN int finish(const Walk& s, unsigned long long& outer) {
    outer = s.rows & ~s.crossed;
    return (s.open & ~s.crossed) ? ENV_OPEN : ENV_OK;
}

// The loops of one entry: n list entries, this one at position `self`.  o.partner(j) makes entry j of the list the partner
// (the caller has checked every entry with member_ok); o.radius(ii) is the radius of [partner; -row ii].
template <class Oracle>
PLP_ENUM_FN void walk(Walk& s, const long long n, const long long self, const double tol, Oracle& o) {
    for (long long j = 0; j < n; ++j) {
        if (j == self) continue;
        if (next_row(s, 0) < 0) break;   // every row is crossed: no test is left
        o.partner(j);
        for (int ii = next_row(s, 0); ii >= 0; ii = next_row(s, ii + 1)) take(s, ii, o.radius(ii), tol);
    }
}

}  // namespace env
}  // namespace plp
