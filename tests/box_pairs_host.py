"""Host build of polytope_amd/csrc/plp_box_pairs.hpp (tests/cabi/box_pairs_host.cpp, g++ -ffp-contract=off) for
tests/test_box_pairs_host.py (CPU: the sequential grid walk against the brute-force definition) and
tests/test_pairs_sparse_gpu.py (the device broad phase against the host's, integer for integer); and the seeded cell
families both files run.  The host grid is built the way polytope_amd.batch._BoxPairs builds the device's: the same
statistics, axis choice and descriptor (batch._locate_boxes / _locate_desc), the sequential count / fill passes."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

from polytope_amd import batch as pb  # noqa: E402

_VP = C.c_void_p
ENGINES = ("NONE", "EMPTY", "LDS", "WIDE", "GROUP", "GENERAL", "LANE", "SPLIT")


def build(tmpdir):
    out = os.path.join(str(tmpdir), "libbox_pairs_host.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-o", out,
                           os.path.join(ROOT, "tests", "cabi", "box_pairs_host.cpp")])
    L = C.CDLL(out)
    L.bph_brute.restype = None
    L.bph_brute.argtypes = [C.c_int, C.c_int, _VP, _VP, C.c_double, C.c_int, _VP, _VP]
    L.bph_walk.restype = None
    L.bph_walk.argtypes = [C.c_int, C.c_int, _VP, _VP, C.c_double, _VP, _VP, _VP, C.c_int, _VP, _VP]
    L.bph_grid_bad.restype = C.c_int
    L.bph_grid_bad.argtypes = [_VP, C.c_int]
    L.bph_grid_count.restype = None
    L.bph_grid_count.argtypes = [_VP, C.c_int, C.c_int, _VP, _VP, C.c_double, _VP, _VP]
    L.bph_grid_fill.restype = None
    L.bph_grid_fill.argtypes = [_VP, C.c_int, C.c_int, _VP, _VP, C.c_double, _VP, _VP, _VP]
    L.bph_plan_pair_list.restype = None
    L.bph_plan_pair_list.argtypes = [C.c_int, C.c_int, C.c_int, C.c_longlong, C.c_char_p, _VP]
    return L


def _p(a):
    return None if a is None else _VP(a.ctypes.data)


def _boxes(lb, ub):
    lb, ub = np.ascontiguousarray(lb, dtype=np.float64), np.ascontiguousarray(ub, dtype=np.float64)
    assert lb.ndim == 2 and lb.shape == ub.shape
    return lb, ub


def brute(L, lb, ub, n1=0, pad=pb._LOCATE_PAD):
    """-> (per_cell int64[n + 1], pairs int32[K, 2]) of the definition: every partner box-tested"""
    lb, ub = _boxes(lb, ub)
    n, d = lb.shape
    per_cell = np.full(n + 1, -7, np.int64)
    L.bph_brute(n, d, _p(lb), _p(ub), float(pad), int(n1), _p(per_cell), None)
    pairs = np.full((int(per_cell[n]), 2), -7, np.int32)
    L.bph_brute(n, d, _p(lb), _p(ub), float(pad), int(n1), _p(per_cell), _p(pairs))
    return per_cell, pairs


class _Numpy(object):
    torch = None


def host_lists(L, lb, ub, pad=pb._LOCATE_PAD, desc=None):
    """The cell lists of the grid batch._BoxPairs would build over these boxes (or over the descriptor given)
    -> (desc, cell_start, cell_items), or None where no axis separates the boxes."""
    lb, ub = _boxes(lb, ub)
    n, d = lb.shape
    if desc is None:
        never = np.zeros(n, bool)
        lb2, ub2, st = pb._locate_boxes(_Numpy(), lb, ub, never, never)
        assert np.array_equal(lb2, lb, equal_nan=True) and np.array_equal(ub2, ub, equal_nan=True)
        desc, axes = pb._locate_desc(n, d, st)
        if desc is None:
            return None
    assert L.bph_grid_bad(_VP(C.addressof(desc)), d) == 0
    G = int(np.prod([desc.res[j] for j in range(desc.naxes)]))
    cell_start, max_len = np.zeros(G + 1, np.int32), np.zeros(1, np.int32)
    L.bph_grid_count(_VP(C.addressof(desc)), n, d, _p(lb), _p(ub), float(pad), _p(cell_start), _p(max_len))
    items, cursor = np.full(max(int(cell_start[G]), 1), -1, np.int32), np.zeros(G, np.int32)
    L.bph_grid_fill(_VP(C.addressof(desc)), n, d, _p(lb), _p(ub), float(pad), _p(cell_start), _p(cursor), _p(items))
    return desc, cell_start, items


def walk(L, lb, ub, lists, n1=0, pad=pb._LOCATE_PAD):
    """-> (per_cell, pairs) of the sequential grid walk over `lists` = host_lists(...)"""
    lb, ub = _boxes(lb, ub)
    n, d = lb.shape
    desc, cell_start, items = lists
    g = _VP(C.addressof(desc))
    per_cell = np.full(n + 1, -7, np.int64)
    L.bph_walk(n, d, _p(lb), _p(ub), float(pad), g, _p(cell_start), _p(items), int(n1), _p(per_cell), None)
    pairs = np.full((int(per_cell[n]), 2), -7, np.int32)
    L.bph_walk(n, d, _p(lb), _p(ub), float(pad), g, _p(cell_start), _p(items), int(n1), _p(per_cell), _p(pairs))
    return per_cell, pairs


def plan(L, n, m_max, d, K, adj_wide=None):
    """plan_pair_list -> dict(engine, gs, rows, grid, block, lds, force_retry, p_lo, p_hi)"""
    out = np.zeros(9, np.int64)
    L.bph_plan_pair_list(n, m_max, d, K, None if adj_wide is None else adj_wide.encode(), _p(out))
    r = dict(zip(("engine", "gs", "rows", "grid", "block", "lds", "force_retry", "p_lo", "p_hi"), (int(v) for v in out)))
    r["engine"] = ENGINES[r["engine"]]
    return r


# ------------------------------------------------------------------------------------------------ cells and their boxes
def box_cells(lo, hi):
    """Axis-aligned boxes [lo_p, hi_p] as cells: rows +e_k x <= hi, -e_k x <= -lo -> A[n, 2d, d], b[n, 2d]"""
    lo, hi = np.asarray(lo, float), np.asarray(hi, float)
    n, d = lo.shape
    A = np.tile(np.vstack([np.eye(d), -np.eye(d)])[None], (n, 1, 1))
    return A, np.concatenate([hi, -lo], 1)


def grid_cells(shape, origin=None, width=1.0):
    """The cells of a box grid with `shape` cells per axis, row-major -> A, b, idx[n, d]"""
    d = len(shape)
    idx = np.stack(np.meshgrid(*[np.arange(s) for s in shape], indexing="ij"), -1).reshape(-1, d)
    lo = idx * float(width) + (0.0 if origin is None else np.asarray(origin, float))
    A, b = box_cells(lo, lo + float(width))
    return A, b, idx


def grid_touching(idx):
    """(i, j), i > j, sorted: the pairs of grid cells whose indices differ by at most 1 on every axis"""
    diff = np.abs(idx[:, None, :] - idx[None, :, :]).max(-1)
    ii, jj = np.nonzero(np.tril(diff <= 1, -1))
    return np.stack([ii, jj], 1).astype(np.int32)


def exact_boxes(A, b, m=None, inflate=0.0):
    """Outer boxes of axis-aligned box cells {A x <= b + inflate} read off their rows (rows +-e_k only); a cell with rows
    of another kind, or without rows, gets the whole space"""
    n, m_max, d = A.shape
    lb, ub = np.full((n, d), -np.inf), np.full((n, d), np.inf)
    for p in range(n):
        mp = m_max if m is None else int(m[p])
        ok = mp > 0
        l, u = np.full(d, -np.inf), np.full(d, np.inf)
        for i in range(mp):
            nz = np.nonzero(A[p, i])[0]
            if nz.size != 1 or abs(A[p, i, nz[0]]) != 1.0:
                ok = False
                break
            k = nz[0]
            if A[p, i, k] > 0:
                u[k] = min(u[k], b[p, i] + inflate)
            else:
                l[k] = max(l[k], -(b[p, i] + inflate))
        if ok:
            lb[p], ub[p] = l, u
    return lb, ub


def scattered_polytopes(rng, n=40, d=3, spread=12.0):
    """n random bounded polytopes of 6..16 rows, scattered over [0, spread]^d so that most pairs are far apart: a cube of
    half-width 0.6..1.2 around a random centre (2d rows) cut by up to 16 - 2d tilted rows -> A[n, 16, d], b, m"""
    m_max = 16
    A, b, m = np.zeros((n, m_max, d)), np.zeros((n, m_max)), np.zeros(n, np.int32)
    for p in range(n):
        c = rng.uniform(0, spread, d)
        h = rng.uniform(0.6, 1.2)
        A[p, :2 * d] = np.vstack([np.eye(d), -np.eye(d)])
        b[p, :2 * d] = np.concatenate([c + h, -(c - h)])
        k = int(rng.integers(0, m_max - 2 * d + 1))
        T = rng.standard_normal((k, d))
        T /= np.linalg.norm(T, axis=1, keepdims=True)
        A[p, 2 * d:2 * d + k] = T
        b[p, 2 * d:2 * d + k] = T @ c + rng.uniform(0.3, 1.0, k) * h
        m[p] = 2 * d + k
    return A, b, m


GAPS = (0.0, 1e-8, 1.7e-7, 1.9e-7, 2.1e-7, 1e-6)


def gap_boxes():
    """Family (d): for each gap g of GAPS the boxes [0, 1] x [10 k, 10 k + 1] and [1 + g, 2 + g] x [10 k, 10 k + 1] (cells
    2 k and 2 k + 1 of one table, d = 2)"""
    lo, hi = [], []
    for k, g in enumerate(GAPS):
        lo += [[0.0, 10.0 * k], [1.0 + g, 10.0 * k]]
        hi += [[1.0, 10.0 * k + 1.0], [2.0 + g, 10.0 * k + 1.0]]
    return box_cells(np.array(lo), np.array(hi))


def fixture_families():
    """The four families of tests/golden/adjacent_sparse.npz -> {name: (A, b, m or None)}"""
    rng = np.random.default_rng(20261020)
    Aa, ba, _ = grid_cells((4, 4, 4))
    Ab, bb, _ = grid_cells((3, 3, 2, 2))
    Ac, bc, mc = scattered_polytopes(rng)
    Ad, bd = gap_boxes()
    return {"a": (Aa, ba, None), "b": (Ab, bb, None), "c": (Ac, bc, mc), "d": (Ad, bd, None)}


def load_fixture():
    """tests/golden/adjacent_sparse.npz -> {name: dict(A, b, m or None, adj uint8[n, n] of the reference's is_adjacent)}"""
    z = np.load(os.path.join(ROOT, "tests", "golden", "adjacent_sparse.npz"))
    out = {}
    for name in "abcd":
        m = z[name + "_m"]
        out[name] = dict(A=z[name + "_A"], b=z[name + "_b"], m=None if m.size == 0 else m, adj=z[name + "_adj"])
    return out


def tril_pairs(M):
    """(i, j), i > j, sorted by (i, j): the nonzeros of the strict lower triangle"""
    ii, jj = np.nonzero(np.tril(np.asarray(M), -1))
    return np.stack([ii, jj], 1).astype(np.int32)


# ------------------------------------------------------------------------------------------------ box families (broad phase)
def box_case_names():
    return ["grid_a", "grid_b", "scattered", "gaps", "n0", "n1", "n2", "slab", "big_box", "halfspace", "empty_nan_inf",
            "all_span", "grid3_4096", "far"]


def box_cases():
    """[(name, lb, ub)]: boxes for the broad-phase tests, every family small"""
    rng = np.random.default_rng(77)
    out = []
    fam = fixture_families()
    for name, key in (("grid_a", "a"), ("grid_b", "b")):
        A, b, m = fam[key]
        out.append((name,) + exact_boxes(A, b, m, 1e-7))
    c = rng.uniform(0, 12, (40, 3))
    h = rng.uniform(0.3, 1.5, (40, 3))
    out.append(("scattered", c - h, c + h))
    A, b = gap_boxes()
    out.append(("gaps",) + exact_boxes(A, b, None, 1e-7))
    A, b, _ = grid_cells((3, 3))
    lb, ub = exact_boxes(A, b)
    for n in (0, 1, 2):
        out.append(("n%d" % n, lb[:n], ub[:n]))
    # a slab across many grid cells beside small cells: it is listed in every cell of its range, reported once per partner
    A, b, _ = grid_cells((12, 12))
    lb, ub = exact_boxes(A, b)
    lb = np.concatenate([[[-1.0, 5.2]], lb, [[3.3, -2.0]]])
    ub = np.concatenate([[[13.0, 5.9]], ub, [[3.6, 14.0]]])
    out.append(("slab", lb, ub))
    # one box over 100 small cells (more than 64 partners), first and last in the table
    A, b, _ = grid_cells((10, 10), width=0.5)
    lb, ub = exact_boxes(A, b)
    out.append(("big_box", np.concatenate([[[-1.0, -1.0]], lb, [[-1.0, -1.0]]]), np.concatenate([[[6.0, 6.0]], ub, [[6.0, 6.0]]])))
    # infinite sides: a half-space among 30 cells
    A, b, _ = grid_cells((6, 5))
    lb, ub = exact_boxes(A, b)
    lb[7] = [-np.inf, -np.inf]
    ub[7] = [2.5, np.inf]
    out.append(("halfspace", lb, ub))
    # empty boxes (lb > ub, on a gridded and on another axis), NaN bounds, a box of infinities
    A, b, _ = grid_cells((5, 5, 2))
    lb, ub = exact_boxes(A, b)
    lb[3], ub[3] = np.inf, -np.inf
    lb[11, 2], ub[11, 2] = 5.0, 4.0
    lb[20, 0] = np.nan
    ub[21, 1] = np.nan
    lb[30], ub[30] = -np.inf, np.inf
    lb[31], ub[31] = np.nan, np.nan
    out.append(("empty_nan_inf", lb, ub))
    # every box spans the domain: no axis separates them
    lb = -1.0 - 0.01 * rng.random((40, 3))
    out.append(("all_span", lb, -lb))
    # enough cells for the kernels' own choice to take the grid walk for some cells and the brute walk for others
    A, b, _ = grid_cells((16, 16, 16))
    lb, ub = exact_boxes(A, b, None, 1e-7)
    lb[100], ub[100] = [-1, 3.1, -1], [17, 3.4, 17]
    out.append(("grid3_4096", lb, ub))
    # coordinates near 1e9 on one axis: the pad goes with the largest coordinate
    A, b, _ = grid_cells((6, 6), origin=(0.0, 1e9))
    out.append(("far",) + exact_boxes(A, b))
    assert [c_[0] for c_ in out] == box_case_names()
    return out
