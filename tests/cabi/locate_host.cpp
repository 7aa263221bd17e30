// Host build of polytope_amd/csrc/plp_locate.hpp (the row test, the cell map, the cell ranges and the sequential count / fill /
// query passes of point location, plp_locate.hip): TEST INFRASTRUCTURE, compiled with g++ -ffp-contract=off by
// tests/locate_host.py.  The device kernels are held against these functions, integer for integer.
#include <stdint.h>

#include "../../polytope_amd/csrc/plp_locate.hpp"

using plp::loc::Grid;

extern "C" {

// out[i] = cell_of(x[i], lo, inv_h, res)
void lh_cells(long long count, const double* x, double lo, double inv_h, int res, int32_t* out) {
    for (long long i = 0; i < count; ++i) out[i] = plp::loc::cell_of(x[i], lo, inv_h, res);
}

// out[q] = the flat cell of column q of X[d][N]
void lh_point_cells(const Grid* g, long long N, const double* X, int32_t* out) {
    for (long long q = 0; q < N; ++q) out[q] = plp::loc::point_cell(*g, X + q, N);
}

int lh_grid_bad(const Grid* g, int d) { return plp::loc::grid_bad(*g, d); }

// listed[p] = 1 and c_lo / c_hi[p][3] = the cell range of polytope p, or listed[p] = 0
void lh_cell_ranges(const Grid* g, int P, int d, const double* lb, const double* ub, double pad, int32_t* listed, int32_t* c_lo,
                    int32_t* c_hi) {
    for (int p = 0; p < P; ++p) {
        int lo[plp::loc::MAX_AXES] = {0, 0, 0}, hi[plp::loc::MAX_AXES] = {0, 0, 0};
        listed[p] = plp::loc::cell_range(*g, d, lb + (size_t)p * d, ub + (size_t)p * d, pad, lo, hi) ? 1 : 0;
        for (int j = 0; j < plp::loc::MAX_AXES; ++j) { c_lo[p * 3 + j] = lo[j]; c_hi[p * 3 + j] = hi[j]; }
    }
}

void lh_grid_count(const Grid* g, int P, int d, const double* lb, const double* ub, double pad, int32_t* cell_start,
                   int32_t* max_len) {
    plp::loc::host_grid_count(*g, P, d, lb, ub, pad, cell_start, max_len);
}

void lh_grid_fill(const Grid* g, int P, int d, const double* lb, const double* ub, double pad, const int32_t* cell_start,
                  int32_t* cursor, int32_t* cell_items) {
    plp::loc::host_grid_fill(*g, P, d, lb, ub, pad, cell_start, cursor, cell_items);
}

int lh_locate(int P, int m_max, int d, const double* A, const double* b, const int32_t* m, long long N, const double* X,
              double tol, const Grid* g, const int32_t* cell_start, const int32_t* cell_items, int32_t* first, int32_t* count) {
    if (d < 1 || d > 16 || P < 0 || m_max < 0 || N < 0) return 2;
    plp::loc::host_locate(P, m_max, d, A, b, m, N, X, tol, g, cell_start, cell_items, first, count);
    return 0;
}

}  // extern "C"
