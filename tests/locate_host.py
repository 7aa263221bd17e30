"""Host build of polytope_amd/csrc/plp_locate.hpp (tests/cabi/locate_host.cpp, g++ -ffp-contract=off) for
tests/test_locate_host.py (CPU: the sequential dense and grid answers against the reference's and against each other) and
tests/test_locate_gpu.py (the device answers against the host's, integer for integer); and the seeded case families both
files run.  The host grid is built the way polytope_amd.batch.locate_grid builds the device's -- the same row
normalisation, axis choice and descriptor (batch._locate_rows / _locate_boxes / _locate_desc) -- with the boxes from the
CPU oracle instead of bbox_batch."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from polytope_amd import batch as pb  # noqa: E402
from polytope_amd._lib import LocateGridDesc  # noqa: E402

_VP = C.c_void_p


def build(tmpdir):
    out = os.path.join(str(tmpdir), "liblocate_host.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-o", out,
                           os.path.join(ROOT, "tests", "cabi", "locate_host.cpp")])
    L = C.CDLL(out)
    L.lh_cells.restype = None
    L.lh_cells.argtypes = [C.c_longlong, _VP, C.c_double, C.c_double, C.c_int, _VP]
    L.lh_point_cells.restype = None
    L.lh_point_cells.argtypes = [_VP, C.c_longlong, _VP, _VP]
    L.lh_grid_bad.restype = C.c_int
    L.lh_grid_bad.argtypes = [_VP, C.c_int]
    L.lh_cell_ranges.restype = None
    L.lh_cell_ranges.argtypes = [_VP, C.c_int, C.c_int, _VP, _VP, C.c_double, _VP, _VP, _VP]
    L.lh_grid_count.restype = None
    L.lh_grid_count.argtypes = [_VP, C.c_int, C.c_int, _VP, _VP, C.c_double, _VP, _VP]
    L.lh_grid_fill.restype = None
    L.lh_grid_fill.argtypes = [_VP, C.c_int, C.c_int, _VP, _VP, C.c_double, _VP, _VP, _VP]
    L.lh_locate.restype = C.c_int
    L.lh_locate.argtypes = [C.c_int, C.c_int, C.c_int, _VP, _VP, _VP, C.c_longlong, _VP, C.c_double, _VP, _VP, _VP, _VP, _VP]
    return L


def _p(a):
    return None if a is None else _VP(a.ctypes.data)


def _g(desc):
    return None if desc is None else _VP(C.addressof(desc))


def _table(A, b, m):
    A = np.ascontiguousarray(A, dtype=np.float64)
    P, m_max, d = A.shape
    b = np.ascontiguousarray(b, dtype=np.float64).reshape(P, m_max)
    m = None if m is None else np.ascontiguousarray(m, dtype=np.int32)
    return A, b, m, (P, m_max, d)


def cells(L, x, lo, inv_h, res):
    x = np.ascontiguousarray(x, dtype=np.float64)
    out = np.empty(x.size, np.int32)
    L.lh_cells(x.size, _p(x), float(lo), float(inv_h), int(res), _p(out))
    return out


def point_cells(L, desc, X):
    X = np.ascontiguousarray(X, dtype=np.float64)
    out = np.empty(X.shape[1], np.int32)
    L.lh_point_cells(_g(desc), X.shape[1], _p(X), _p(out))
    return out


def cell_ranges(L, desc, lb, ub, pad=pb._LOCATE_PAD):
    lb, ub = np.ascontiguousarray(lb, dtype=np.float64), np.ascontiguousarray(ub, dtype=np.float64)
    P, d = lb.shape
    listed, lo, hi = np.empty(P, np.int32), np.empty((P, 3), np.int32), np.empty((P, 3), np.int32)
    L.lh_cell_ranges(_g(desc), P, d, _p(lb), _p(ub), float(pad), _p(listed), _p(lo), _p(hi))
    return listed.astype(bool), lo, hi


def locate(L, A, b, X, abs_tol=1e-7, m=None, grid=None):
    """-> (first, count) of the sequential restatement; grid: None (dense) or a HostGrid of kind "grid"."""
    A, b, m, (P, m_max, d) = _table(A, b, m)
    X = np.ascontiguousarray(X, dtype=np.float64)
    N = X.shape[1]
    first, count = np.full(N, -7, np.int32), np.full(N, -7, np.int32)
    use = grid is not None and grid.kind == "grid"
    rc = L.lh_locate(P, m_max, d, _p(A), _p(b), _p(m), N, _p(X), float(abs_tol), _g(grid.desc) if use else None,
                     _p(grid.cell_start) if use else None, _p(grid.cell_items) if use else None, _p(first), _p(count))
    assert rc == 0
    return first, count


class _Numpy(object):
    torch = None


def oracle_boxes(O, An, bn, m):
    """lb[P, d], ub[P, d], status[P] of the normalised relaxed rows from the CPU oracle (status 1: no box -- the oracle
    reports a failed LP, or the polytope is empty or flat, where bbox_batch hands the polytope back as well)."""
    P, m_max, d = An.shape
    lb, ub, status = np.zeros((P, d)), np.zeros((P, d)), np.zeros(P, np.int32)
    for p in range(P):
        mp = m_max if m is None else int(m[p])
        if mp == 0:
            status[p] = 1
            continue
        st, r, _ = O.cheby(An[p, :mp], bn[p, :mp])
        if st != 0 or not (r >= 1e-6):
            status[p] = 1
            continue
        lo, hi, bad = O.bounding_box(An[p, :mp], bn[p, :mp])
        lb[p], ub[p], status[p] = lo, hi, 1 if bad else 0
    return lb, ub, status


def host_grid(L, O, A, b, m=None, abs_tol=1e-7, max_items=pb._LOCATE_MAX_ITEMS, max_list=pb._LOCATE_MAX_LIST):
    """batch.locate_grid with the oracle's boxes and the sequential count / fill -> batch.LocateGrid with numpy lists
    (and .lb / .ub: the boxes the lists were built from)."""
    A, b, m, (P, m_max, d) = _table(A, b, m)

    def dense(reason):
        return pb.LocateGrid("dense", abs_tol, (P, m_max, d), reason=reason)
    if P == 0 or m_max == 0:
        return dense("no rows")
    if m_max > pb.MAX_M:
        return dense("rows")
    be = _Numpy()
    An, bn, every, nowhere = pb._locate_rows(be, A, b, m, abs_tol)
    lb, ub, status = oracle_boxes(O, An, bn, m)
    lb, ub, st = pb._locate_boxes(be, lb, ub, every | (status != 0), nowhere)
    if st[4, 0] > max_list:
        return dense("everywhere")
    desc, axes = pb._locate_desc(P, d, st)
    if desc is None:
        return dense("no axis")
    G = int(np.prod([a[3] for a in axes]))
    cell_start, max_len = np.zeros(G + 1, np.int32), np.zeros(1, np.int32)
    L.lh_grid_count(_g(desc), P, d, _p(lb), _p(ub), pb._LOCATE_PAD, _p(cell_start), _p(max_len))
    n_items, longest = int(cell_start[G]), int(max_len[0])
    if n_items > max_items or longest > max_list:
        return dense("budget")
    items, cursor = np.full(n_items, -1, np.int32), np.zeros(G, np.int32)
    L.lh_grid_fill(_g(desc), P, d, _p(lb), _p(ub), pb._LOCATE_PAD, _p(cell_start), _p(cursor), _p(items))
    g = pb.LocateGrid("grid", abs_tol, (P, m_max, d), desc, cell_start, items, n_items, longest)
    g.lb, g.ub = lb, ub
    return g


# ------------------------------------------------------------------------------------------------ cases
def dense_ppl(d):
    """Points per lane of the dense location kernel (csrc/plp_locate.hip: launch_locate_d), so that N can straddle a
    wavefront's share of the points.  A copy: if the kernel's table moves, the N cases below only stop straddling it."""
    return 8 if d <= 3 else 6 if d <= 8 else 4 if d == 9 else 3 if d <= 12 else 2


def case_names():
    """the names of cases(), in order, without building anything (test ids at collection time)"""
    names = ["d%d" % d for d in range(1, 17)]
    for d in (3, 6):
        ppl = dense_ppl(d)
        names += ["d%d_N%d" % (d, N) for N in (0, 1, 63, 64, 65, 64 * ppl - 1, 64 * ppl + 1)]
    names += ["P0", "P1", "P2", "ragged_m0_first", "ragged_m0_middle", "ragged_m0_last", "overlap_dup", "outside_inf_nan",
              "outside_inf_nan_m0", "halfspaces", "all_span", "list_cap", "rescaled", "zero_rows", "soak_dup", "soak_flat",
              "structured", "cube_dup_d3", "cube_dup_d4", "far_tilted"]
    return names


def _cells_table(d, per_axis, rng, lo=-1.0, hi=1.0, jitter=0.0):
    """per_axis^d axis-aligned boxes tiling [lo, hi]^d (rows +-e_k), in row-major order -> A[P, 2d, d], b[P, 2d]"""
    edges = np.linspace(lo, hi, per_axis + 1)
    idx = np.stack(np.meshgrid(*[np.arange(per_axis)] * d, indexing="ij"), -1).reshape(-1, d)
    P = idx.shape[0]
    A = np.tile(np.vstack([np.eye(d), -np.eye(d)])[None], (P, 1, 1))
    b = np.concatenate([edges[idx + 1], -edges[idx]], 1) + jitter * rng.random((P, 2 * d))
    return A, b


def _points(rng, d, N, scale=1.5):
    return np.ascontiguousarray(rng.uniform(-scale, scale, (d, N)))


def cases():
    """[(name, A, b, m, X, abs_tol)]: the families of tests/test_locate_gpu.py; every one small."""
    import soak_lane
    from structured_cases import structured_polytopes
    from degenerate_cases import degenerate_lps
    rng = np.random.default_rng(2026)
    tol = 1e-7
    out = []
    # d = 1..16, P = 5, m_max = 6, N = 200: a box around a random centre (2 rows on each of up to 3 axes)
    for d in range(1, 17):
        P, m_max, N = 5, 6, 200
        A = np.zeros((P, m_max, d))
        b = np.zeros((P, m_max))
        m = np.zeros(P, np.int32)
        for p in range(P):
            ax = rng.permutation(d)[:min(d, 3)]
            c = rng.uniform(-1, 1, d)
            k = 0
            for a in ax:
                A[p, k, a], b[p, k] = 1.0, c[a] + 0.6
                A[p, k + 1, a], b[p, k + 1] = -1.0, -(c[a] - 0.6)
                k += 2
            if d > 1 and k < m_max:     # a tilted row where there is room
                A[p, k] = rng.standard_normal(d)
                b[p, k] = A[p, k] @ c + 0.5 * np.linalg.norm(A[p, k])
                k += 1
            m[p] = k
        out.append(("d%d" % d, A, b, m, _points(rng, d, N), tol))
    # N around the wavefront's share (dense kernel: 64 x PPL points per wavefront pass), d = 3 and d = 6
    for d in (3, 6):
        A, b = _cells_table(d, 2, rng)
        ppl = dense_ppl(d)
        for N in (0, 1, 63, 64, 65, 64 * ppl - 1, 64 * ppl + 1):
            out.append(("d%d_N%d" % (d, N), A, b, None, _points(rng, d, N, 1.2), tol))
    # P = 0, 1, 2
    A, b = _cells_table(2, 2, rng)
    for P in (0, 1, 2):
        out.append(("P%d" % P, A[:P], b[:P], None, _points(rng, 2, 100, 1.2), tol))
    # ragged m, with m[p] == 0 first / in the middle / last
    A, b = _cells_table(3, 3, rng)
    for pos, name in ((0, "first"), (13, "middle"), (26, "last")):
        m = rng.integers(3, 7, 27).astype(np.int32)
        m[pos] = 0
        out.append(("ragged_m0_%s" % name, A, b, m, _points(rng, 3, 300, 1.2), tol))
    # overlapping and duplicated polytopes
    A, b = _cells_table(2, 4, rng, jitter=0.3)
    A, b = np.concatenate([A, A[::3]]), np.concatenate([b, b[::3]])
    out.append(("overlap_dup", A, b, None, _points(rng, 2, 500, 1.3), tol))
    # points outside every box and outside the domain on each side; +-inf and NaN coordinates
    A, b = _cells_table(3, 4, rng)
    X = _points(rng, 3, 400, 1.0)
    X[:, :60] = rng.uniform(-5, 5, (3, 60))
    for k in range(3):
        X[k, 60 + 2 * k], X[k, 61 + 2 * k] = -3.0, 3.0
        X[k, 70 + 3 * k], X[k, 71 + 3 * k], X[k, 72 + 3 * k] = np.inf, -np.inf, np.nan
    X[:, 90] = np.nan
    out.append(("outside_inf_nan", A, b, None, X, tol))
    m = np.full(64, 6, np.int32)
    m[5] = 0                         # a rowless polytope contains the NaN points too
    out.append(("outside_inf_nan_m0", A, b, m, X, tol))
    # half-spaces among bounded cells (infinite box sides)
    A, b = _cells_table(2, 5, rng)
    m = np.full(25, 4, np.int32)
    m[::4] = rng.integers(1, 4, m[::4].size)
    out.append(("halfspaces", A, b, m, _points(rng, 2, 500, 2.0), tol))
    # every polytope spans the domain: no axis separates them, the grid is declined
    d = 3
    A = rng.standard_normal((40, 8, d))
    A[:, :6] = np.vstack([np.eye(d), -np.eye(d)])[None]
    b = np.ones((40, 8)) + 0.01 * rng.random((40, 8))
    out.append(("all_span", A, b, None, _points(rng, d, 300, 1.2), tol))
    # a single list above the cap: 1100 copies of one small cell beside a spread of others
    A1, b1 = _cells_table(2, 6, rng)
    Ac = np.tile(A1[:1], (1100, 1, 1))
    bc = np.tile(b1[:1], (1100, 1))
    out.append(("list_cap", np.concatenate([A1, Ac]), np.concatenate([b1, bc]), None, _points(rng, 2, 200, 1.1), tol))
    # rows rescaled by 1e-6, probes up to abs_tol / |a| outside the unrelaxed facet
    A, b = _cells_table(2, 4, rng)
    s = np.where(rng.random(b.shape) < 0.4, 1e-6, 1.0)
    A, b = A * s[:, :, None], b * s
    X = _points(rng, 2, 300, 1.0)
    # (facet x_0 <= edge of rescaled rows: the relaxed facet sits at edge + abs_tol / 1e-6 = edge + 0.1)
    X[0, :100] = rng.choice(np.linspace(-1, 1, 5), 100) + rng.uniform(-0.1, 0.1, 100)
    X[1, 100:200] = rng.choice(np.linspace(-1, 1, 5), 100) + rng.uniform(-0.1, 0.1, 100)
    out.append(("rescaled", A, b, None, X, tol))
    # zero rows with b + abs_tol on both sides of 0
    A, b = _cells_table(2, 4, rng)
    A = np.concatenate([A, np.zeros((16, 1, 2))], 1)
    b = np.concatenate([b, rng.choice([1.0, 0.0, -tol, -2 * tol, -0.5 * tol, 1e-300], (16, 1))], 1)
    out.append(("zero_rows", A, b, None, _points(rng, 2, 300, 1.1), tol))
    # dup and flat families: soak_lane, the structured (16, 3) set, duplicated cube faces
    for fam in ("dup", "flat"):
        A, b, m = soak_lane.make(rng, 24, 12, 3, fam)
        out.append(("soak_" + fam, A, b, m, _points(rng, 3, 400, 2.0), tol))
    A, b, _ = structured_polytopes(32)
    out.append(("structured", A, b, None, _points(rng, 3, 500, 2.5), tol))
    for d in (3, 4):
        rows = [(G, h) for kind, _, G, h in degenerate_lps(dims=(d - 1,), reps=6) if kind == "cube_dup_F1"]
        A = np.stack([G for G, _ in rows]) + 0.0
        b = np.stack([h for _, h in rows]) + rng.uniform(0, 0.5, (len(rows), 1))
        out.append(("cube_dup_d%d" % d, A, b, None, _points(rng, d, 300, 1.5), tol))
    # cells near the origin on one axis and about 1e9 away on the other, each with a tilted row: the rounding of a . x goes
    # with the far coordinate, and so does the pad of the box
    A, b = _cells_table(2, 4, rng)
    b[:, 1] += 1e9
    b[:, 3] -= 1e9
    t = rng.standard_normal((16, 1, 2))
    cen = np.stack([(b[:, 0] - b[:, 2]) / 2, (b[:, 1] - b[:, 3]) / 2], 1)
    A = np.concatenate([A, t], 1)
    b = np.concatenate([b, np.einsum("pik,pk->pi", t, cen) + 0.1 * np.linalg.norm(t, axis=2)], 1)
    X = _points(rng, 2, 400, 1.1)
    X[1] += 1e9
    out.append(("far_tilted", A, b, None, X, tol))
    assert [c[0] for c in out] == case_names()
    return out
