// Host build of polytope_amd/csrc/plp_box_pairs.hpp (the candidate rule of the sparse pair calls, its brute-force and grid
// restatements) with the cell lists of plp_locate.hpp, and of plan_pair_list (plp_lp_plan.hpp, a pure host header): TEST
// INFRASTRUCTURE, compiled with g++ -ffp-contract=off by tests/box_pairs_host.py.  The device kernels of plp_box_pairs.hip
// are held against these functions, integer for integer.
#include <stdint.h>

#include "../../polytope_amd/csrc/plp_box_pairs.hpp"
#include "../../polytope_amd/csrc/plp_lp_plan.hpp"

using plp::loc::Grid;

extern "C" {

// per_cell[n + 1]; pairs[per_cell[n]][2] or NULL (count only)
void bph_brute(int n, int d, const double* lb, const double* ub, double pad, int n1, int64_t* per_cell, int32_t* pairs) {
    plp::bp::host_brute(n, d, lb, ub, pad, n1, per_cell, pairs);
}

void bph_walk(int n, int d, const double* lb, const double* ub, double pad, const Grid* g, const int32_t* cell_start,
              const int32_t* cell_items, int n1, int64_t* per_cell, int32_t* pairs) {
    plp::bp::host_walk(n, d, lb, ub, pad, *g, cell_start, cell_items, n1, per_cell, pairs);
}

int bph_grid_bad(const Grid* g, int d) { return plp::loc::grid_bad(*g, d); }

void bph_grid_count(const Grid* g, int P, int d, const double* lb, const double* ub, double pad, int32_t* cell_start,
                    int32_t* max_len) {
    plp::loc::host_grid_count(*g, P, d, lb, ub, pad, cell_start, max_len);
}

void bph_grid_fill(const Grid* g, int P, int d, const double* lb, const double* ub, double pad, const int32_t* cell_start,
                   int32_t* cursor, int32_t* cell_items) {
    plp::loc::host_grid_fill(*g, P, d, lb, ub, pad, cell_start, cursor, cell_items);
}

// plan_pair_list(n, m_max, d, K) under PLP_ADJ_WIDE = adj_wide (NULL: unset) -> out: engine (LpEngine), gs, rows, grid,
// block, LDS bytes, force_retry, p_lo, p_hi
void bph_plan_pair_list(int n, int m_max, int d, long long K, const char* adj_wide, long long* out) {
    plp::LpEnv e;
    e.adj_wide = adj_wide;
    const plp::PairPlan p = plp::plan_pair_list(n, m_max, d, K, e);
    const long long v[] = {p.first.engine, p.first.gs, p.first.rows, p.first.grid, p.first.block, (long long)p.first.lds,
                           p.force_retry,  p.p_lo,     p.p_hi};
    for (int k = 0; k < 9; ++k) out[k] = v[k];
}

}  // extern "C"
