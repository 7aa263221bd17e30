// plp_kernels.hpp -- host-side launchers of the HIP kernels (internal to libplp_hip.so).
// Every launcher returns 0, or 2 for an unsupported size; launches are asynchronous on `st`.
#pragma once
#include "plp_common.hpp"

struct plp_locate_grid;  // include/plp.h

namespace plp {

// The stand-alone LP family (plp_lp.hip).  Which kernels a call runs is decided by plan_lp / plan_cheby / plan_bbox /
// plan_pairs (plp_lp_plan.hpp); these carry the plan out (the launchers of the single engines: plp_lp_launch.hpp).
// launch_lp_phase: phase 0 everything; phase 1 the fast kernels only, *more = 1 when LPs they hand over (status ST_RETRY)
// may exist; phase 2 the general kernel's pass over exactly those.  launch_lp is phase 0.
int launch_lp(long long B, int m_max, int n, const double* c, const double* G, const double* h, const int* mrows,
              double* x, double* fun, int* status, int* iters, hipStream_t st);
int launch_lp_phase(long long B, int m_max, int n, const double* c, const double* G, const double* h, const int* mrows,
                    double* x, double* fun, int* status, int* iters, hipStream_t st, int phase, int* more);

int launch_cheby(long long B, int m_max, int d, const double* A, const double* b, const int* mrows, double* r,
                 double* xc, int* status, hipStream_t st);

// Chebyshev LPs on row subsets rows[off[p] .. off[p+1]) of one resident table (region_diff's search): LPs sel[0..nlp)
// of the batch; out[p] = radius as cheby_ball reads it (0 unless optimal with r >= 0).  plp_rdiff.hip / plp_lds.hip
int launch_cheby_gather_r(int d, long long n0, long long n1, long long n2, const int* off, const int* rows, const int* sel,
                          const double* A, const double* b, double* out, hipStream_t st);
// the LP server of a region_diff search (plp_rdiff.hip, d <= 4): one resident launch, batches through a host-mapped mailbox
int launch_rdiff_server(int d, int nwg, const unsigned long long* mail, const int* rec, void* out, unsigned long long* alive,
                        unsigned long long* dstate, const double* A, const double* b, unsigned long long last_word,
                        unsigned idle_polls, hipStream_t st);
void launch_rdiff_publish(long long n, const double* src, double* host_out, unsigned long long* host_flag,
                          unsigned long long seq, hipStream_t st);
// lists of at most 64 rows, d = 5..16: one LP per wavefront (plp_wide.hip); returns 1 when it does not apply
int launch_cheby_gather_w(int d, long long nlp, const int* off, const int* rows, const int* sel, const double* A,
                          const double* b, double* out, hipStream_t st);
int launch_cheby_gather_lds(int d, int m_cap, long long nlp, const int* off, const int* rows, const int* sel,
                            const double* A, const double* b, double* out, hipStream_t st);

// fused reduce() of polytopes with more than 64 rows: rows and dictionary in LDS, keep = ceil(m_max / 64) words per
// polytope (plp_lds.hip); returns 2 when a polytope does not fit the CU's LDS
// one Fourier-Motzkin elimination step (plp_fm.hip): emit = 0 writes count[] (|N| + |P| |Q| per polytope), emit = 1 the
// rows into Aout[B][mo_max][d - (col >= 0)], bout, mout (-1: more than mo_max rows).  2: unsupported size
int launch_fm(int emit, long long B, int m_max, int d, const double* A, const double* b, const int* mrows,
              const unsigned long long* keep, int kw, const int* flags, int col, int first, double abs_tol, int* count,
              int mo_max, double* Aout, double* bout, int* mout, hipStream_t st);
size_t fm_lds_bytes(int m_max, int d);
// Monte-Carlo volume (plp_volume.hip): hits[B] = samples of default_rng's PCG64 stream (state / inc: two words per polytope,
// low first) in the box [lb, ub] that lie strictly inside; flags[B]: vol::VF_*.  Zeroes hits and flags on `st`.  2: unsupported size
int launch_volume_hits(long long B, int m_max, int d, const double* A, const double* b, const int* mrows, const double* lb,
                       const double* ub, const unsigned long long* state, const unsigned long long* inc, long long N,
                       unsigned* hits, int* flags, hipStream_t st);
// support functions in K directions per polytope, rows staged once (plp_support.hip; d <= 4, m_max <= 64): val[B][K],
// x[B][K][d] (or nullptr), status[B][K] (0 optimum, 3 unbounded, 1 handed back).  2: unsupported size
int launch_support(long long B, int m_max, int d, const double* A, const double* b, const int* mrows, int K, const double* C,
                   int c_shared, const double* xc, double* val, double* x, int* status, hipStream_t st);
// nearest points / Euclidean distances of K points per polytope, rows staged once per (tile, K-chunk) at unit norm
// (plp_nearest.hip; d <= 4, m_max <= 64): dist[B][K], status[B][K] (0 optimum, 2 empty, 1 handed back); x[B][K][d],
// face[B][K], lam[B][K][d] each or nullptr.  2: unsupported size
int launch_nearest(long long B, int m_max, int d, const double* A, const double* b, const int* mrows, int K, const double* X,
                   int x_shared, double* dist, double* x, unsigned long long* face, double* lam, int* status, hipStream_t st);
// closest points / Euclidean distances of K listed cell pairs of a table of n cells, two lanes per pair (plp_pair_dist.hip;
// d <= 4, m_max <= 64): dist[K], status[K] (0 settled, 1 handed back, 3 unbounded, 255 a bad pair); lb[K], x[K][d], y[K][d]
// each or nullptr.  2: unsupported size
int launch_pair_dist(int n, int m_max, int d, const double* A, const double* b, const int* mrows, const double* xc, long long K,
                     const int* pairs, double* dist, double* lb, double* x, double* y, int* status, hipStream_t st);
// vertices of small polytopes by enumeration of bases, one polytope per wavefront (plp_extreme.hip; d <= 4, m_max <= 64):
// V[B][v_max][d], count[B], basis[B][v_max][d] (or nullptr), status[B] (0, 1 overflow, 2 empty).  2: unsupported size
int launch_extreme(long long B, int m_max, int d, const double* A, const double* b, const int* mrows,
                   const unsigned long long* keep, int v_max, double* V, int* count, int* basis, int* status, hipStream_t st);
// facets of small point sets by enumeration of hyperplanes, one point set per wavefront (plp_hull_enum.hip; d <= 4,
// n_max <= 64): Ao[B][f_max][d], bo[B][f_max], on[B][f_max], count[B], basis[B][f_max][d] (or nullptr), status[B] (0,
// 1 overflow, 2 flat).  2: unsupported size
int launch_hull_enum(long long B, int n_max, int d, const double* X, const int* npts, const unsigned long long* keep, int f_max,
                     double* Ao, double* bo, unsigned long long* on, int* count, int* basis, int* status, hipStream_t st);
// exact volumes and facet areas of small polytopes by Lasserre's facet recursion, one polytope per wavefront
// (plp_volume_exact.hip; d <= 4, m_max <= 64): volume[B], area[B][m_max] (or nullptr), status[B] (0, 1 unbounded, 2 empty);
// keep, xc[B][d], scale[B] may be nullptr.  2: unsupported size
int launch_volume_exact(long long B, int m_max, int d, const double* A, const double* b, const int* mrows,
                        const unsigned long long* keep, const double* xc, const double* scale, double* volume, double* area,
                        int* status, hipStream_t st);
// B set differences, one whole region_diff search per wavefront (plp_rdiff_batch.hip; d <= 4, the caps of
// plp_rdiff_batch.hpp): the pieces as row lists kind[B][p_max], off[B][p_max + 1], rows[B][r_max], count / nrows / nlp /
// status[B], mi[B][n_max], src[B][M_max].  2: unsupported size
int launch_rdiff_batch(long long B, int m_max, int d, const double* A, const double* b, const int* m, long long Nc, int mc_max,
                       const double* CA, const double* Cb, const int* mc, const int* cell_off, const int* cell_idx,
                       double abs_tol, int max_lps, int p_max, int r_max, int n_max, int M_max, int* kind, int* off, int* rows,
                       int* count, int* nrows, int* nlp, int* status, int* mi, int* src, hipStream_t st);
// The facet tests of envelope() for B regions given as index lists into a packed member table, one list entry per
// wavefront (plp_envelope.hip; d <= 8, members of 1 .. 63 rows): outer / status / nlp[L].  2: unsupported size
int launch_envelope_cross(long long C, int mc_max, int d, const double* A, const double* b, const int* mc, long long B,
                          const int* reg_off, long long L, const int* mem_idx, double abs_tol, unsigned long long* outer,
                          int* status, int* nlp, hipStream_t st);
// The iterative-hull projection of B polytopes onto k of their coordinates, one polytope per wavefront (plp_projhull.hip;
// k <= 3, d <= 16, m_max <= 64, f_max <= 128): keep[k] HOST integers; Ao[B][f_max][k], bo / on[B][f_max], count[B],
// V[B][64][k], nv[B], X[B][64][d] (or nullptr), vmask / nlp / status[B].  2: unsupported size
int launch_projhull(long long B, int m_max, int d, int k, const double* A, const double* b, const int* mrows, const int* keep,
                    const double* xc, int f_max, int max_lps, double* Ao, double* bo, unsigned long long* on, int* count, double* V,
                    int* nv, double* X, unsigned long long* vmask, int* nlp, int* status, hipStream_t st);
int launch_reduce_lds(long long B, int m_max, int d, const double* A, const double* b, const int* mrows, double abs_tol,
                      unsigned long long* keep, int* flags, double* r, double* xc, int* nlp, hipStream_t st);

// bounding boxes, Chebyshev LP + 2d LPs from its centre per polytope (m_max = 1..64): status 0 = lb/ub valid, 1 = polytope
// left to the generic LPs.
// What the fused bounding-box kernels hand to the verifier (plp_verify.hip), per box LP (2d per polytope, lower_0, upper_0,
// lower_1, ...): `basis8` -- its final basis, d signed bytes (>= 0: an active row; -1 - j: the free variable x'_j left at the
// centre) -- with `centre` (d doubles per polytope), or `xfin` -- the point it ended on (d doubles; the one-LP-per-lane
// kernel, whose walk has no basis of d entries when it ends on a face).  Which of the two a call fills: BoxPlan::handover.
struct BoxHandover {
    signed char* basis8;
    double* centre;
    double* xfin;
};
int launch_bbox(long long B, int m_max, int d, const double* A, const double* b, const int* mrows, double* lb,
                double* ub, int* status, hipStream_t st, const BoxHandover* ho = nullptr);

// adjacency of all pairs of n cells (2*m_max <= 64) into the n x n matrix adj (compact == nullptr),
// or of the pairs p_lo <= p < p_hi, p = i (i - 1) / 2 + j, j < i, into compact[p - p_lo]
// a pair counts iff the Chebyshev radius of the two stacked cells, each b inflated by `inflate`, exceeds `thresh`
// cross_n1 > 0 (compact only): the table holds two lists, n1 cells then n - n1 cells, and pair p = a (n - n1) + c is cell a
// of the first list stacked on cell c of the second (p_lo <= p < p_hi within [0, n1 (n - n1)))
// careful_scratch (pair_careful_scratch_bytes() bytes of device memory, or nullptr): a pair whose stacked LP the engines end
// "unbounded" or at their iteration limit is written as PAIR_OPEN and solved again by the careful engine of plp_verify.hpp in
// a launch that follows (launch_careful_pairs) -- on rows a hair apart the engines' "unbounded" can be a bounded LP, and the
// stand-alone Chebyshev batches send every such answer there too; nullptr: those pairs count as "no" (PLP_VERIFY=0)
constexpr unsigned char PAIR_OPEN = 2;
int launch_adjacent(int n, int m_max, int d, const double* A, const double* b, const int* mrows, double inflate,
                    double thresh, unsigned char* adj, long long p_lo, long long p_hi, unsigned char* compact,
                    hipStream_t st, int cross_n1 = 0, void* careful_scratch = nullptr);
size_t pair_careful_scratch_bytes();
// what launch_adjacent wrote with the pairs marked PAIR_OPEN: those pairs decided by the careful engine, one pair per thread
void launch_careful_pairs(int n, int m_max, int d, const double* A, const double* b, const int* mrows, double inflate,
                          double thresh, unsigned char* adj, long long p_lo, long long p_hi, unsigned char* compact,
                          int cross_n1, void* scratch, hipStream_t st, const int* list = nullptr);
// the listed form (plp_pair_list): out[t] = the verdict the calls above give pair (list[2 t], list[2 t + 1]), through the same
// engines (plan_pair_list picks among them by K) and the same careful pass; PAIR_BAD for a pair with an index outside
// [0, n) or two equal ones, for which nothing is read
int launch_pair_list(int n, int m_max, int d, const double* A, const double* b, const int* mrows, double inflate, double thresh,
                     long long K, const int* list, unsigned char* out, hipStream_t st, void* careful_scratch = nullptr);

// Fused reduce() of up to 64 rows (plp_reduce.hip).  The batch, the outputs, and what the fast kernels report besides:
struct ReduceArgs {
    long long B;
    int m_max;
    const double* A;
    const double* b;
    const int* mrows;
    double abs_tol;
    unsigned long long* keep;
    int* flags;
    double* r;
    double* xc;
    int* nlp;
    unsigned long long* ctr;          // the context's counter of simplex runs (plp_reduce_counters), or nullptr
    unsigned long long* retry_word;   // the call's word of the context's ring, or nullptr: the fast kernels raise it to
    unsigned long long epoch;         // `epoch` when they hand a polytope back (RF_RETRY), and the second pass leaves at once
                                      // when it does not hold that value
};
// phase 0: everything (the plan's first launch, then -- when the plan asks for it -- the general kernel's second pass that
// redoes what the first flagged RF_RETRY);  phase 1: the first launch only -- the caller looks at the flags itself and asks
// for phase 2 (that second pass) when it finds RF_RETRY.  Returns 0, or 2 for an unsupported size.
int launch_reduce(int d, const ReduceArgs& a, int phase, hipStream_t st);

// `scratch` (contains_scratch_bytes(P, m_max) bytes of device memory, or nullptr): the per-row thresholds of the
// comparison form (plp_points.hip); without it the subtraction stays in the kernel
int launch_contains(int P, int m_max, int d, const double* A, const double* b, const int* mrows, long long N,
                    const double* X, double abs_tol, int mode, unsigned char* out, void* scratch, hipStream_t st);
size_t contains_scratch_bytes(int P, int m_max);

// point location (plp_locate.hip): first[N] = the first polytope containing each point or -1, count[N] (or nullptr) how
// many do; grid == nullptr: every polytope against every point, else the cell lists cell_start / cell_items of the grid.
// The grid descriptors are host pointers (passed to the kernels by value).  2: unsupported size or a bad descriptor;
// 3 (count / fill): clearing the counters failed (a HIP error)
int launch_locate(int P, int m_max, int d, const double* A, const double* b, const int* mrows, long long N, const double* X,
                  double abs_tol, const plp_locate_grid* grid, const int* cell_start, const int* cell_items, int* first,
                  int* count, hipStream_t st);
// cell_start[G + 1]: exclusive prefix sums of the cells' list lengths, max_len[1]: the longest list
int launch_locate_grid_count(int P, int d, const double* lb, const double* ub, double pad, const plp_locate_grid* grid,
                             int* cell_start, int* max_len, hipStream_t st);
// cell_items[cell_start[G]], every list ascending; cursor[G]: scratch
int launch_locate_grid_fill(int P, int d, const double* lb, const double* ub, double pad, const plp_locate_grid* grid,
                            const int* cell_start, int* cursor, int* cell_items, hipStream_t st);

// the broad phase of the sparse pair calls (plp_box_pairs.hip): per_cell[n + 1], the exclusive prefix sums of the cells'
// numbers of partners whose padded box meets theirs; the pairs of cells [cell_lo, cell_hi) at per_cell[i] - per_cell[cell_lo].
// grid == nullptr: every partner box-tested.  Return 0, 2 for bad sizes, 3 when hipMemsetAsync failed.
int launch_box_pairs_count(int n, int d, const double* lb, const double* ub, double pad, const plp_locate_grid* grid,
                           const int* cell_start, const int* cell_items, int n1, long long* per_cell, hipStream_t st);
int launch_box_pairs_fill(int n, int d, const double* lb, const double* ub, double pad, const plp_locate_grid* grid,
                          const int* cell_start, const int* cell_items, int n1, const long long* per_cell, int cell_lo,
                          int cell_hi, int* pairs, hipStream_t st);

// the stacks of listed cell pairs (plp_pair_stack.hip; the rule: plp_pair_stack.hpp): A_s[K][2 m_max][d], b_s[K][2 m_max],
// m_s[K].  Return 0, 2 for sizes outside 2 m_max <= 64, d <= 16.  launch_pair_bad: the outputs of the bad pairs of a chunk of
// plp_intersect_pairs_dev (m_out may be NULL).
int launch_pair_stacks(int n, int m_max, int d, const double* A, const double* b, const int* m, long long K, const int* pairs,
                       double* A_s, double* b_s, int* m_s, hipStream_t st);
void launch_pair_bad(int n, int d, long long K, const int* pairs, unsigned long long* keep, int* flags, double* r, double* xc,
                     int* nlp, int* ms, int* m_out, hipStream_t st);

int launch_assign(long long N, int d, const double* X, int F, const double* normals, const double* offsets,
                  double abs_tol, int* facet_of_point, double* dist, long long* argmax, double* maxd,
                  void* scratch, size_t scratch_bytes, hipStream_t st);
size_t assign_scratch_bytes(long long N, int F);

// quickhull outside sets on resident points (plp_hull.hip)
int launch_hull_reassign(long long N, int d, const double* X, int* owner, double* dist, const unsigned char* dead,
                         int new_id0, int n_new, const double* normals, const double* offsets, double abs_tol,
                         long long* argmax, double* maxd, long long* count, hipStream_t st);
void launch_hull_mark(int n, const int* ids, unsigned char* dead, hipStream_t st);
void launch_hull_drop(long long n, const long long* idx, int* owner, hipStream_t st);

int launch_selftest(int gs, double* out_d, unsigned* out_u, hipStream_t st);

// the verifier behind the LP / Chebyshev / bounding-box batches (plp_verify.hip): `scratch` holds verify_scratch_bytes(nlp,
// m_max) bytes, `parity` alternates between the launches of a stream (which of its two list counters this one uses)
size_t verify_scratch_bytes(long long nlp, int m_max);
bool verify_enabled();
int launch_verify_lp(long long B, int m_max, int n, const double* c, const double* G, const double* h, const int* mrows,
                     double* x, double* fun, int* status, void* scratch, int parity, hipStream_t st);
int launch_verify_cheby(long long B, int m_max, int d, const double* A, const double* b, const int* mrows, double* r,
                        double* xc, int* status, void* scratch, int parity, hipStream_t st);
int launch_verify_box(long long B, int m_max, int d, const double* A, const double* b, const int* mrows, double* lb, double* ub,
                      int* status, const signed char* basis8, const double* centre, const double* xfin, void* scratch,
                      int parity, hipStream_t st);

}  // namespace plp
