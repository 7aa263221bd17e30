"""GPU: the sparse pair screens (csrc/plp_box_pairs.hip, the listed pair engines, batch.adjacent_pairs_sparse /
overlap_pairs_sparse / overlap_cross_sparse / box_pairs / pair_verdicts, prop2partition.adjacency_sparse / overlap_sparse).
Everything is integer equality: the sparse calls against the nonzeros of the dense calls (on a stream of
their own: tests/test_streams_pairs_sparse_gpu.py), the device broad phase (every walk)
against the host's brute force (tests/box_pairs_host.py), pair_verdicts against the dense entries; the reference's answers
(tests/golden/adjacent_sparse.npz) may be missed only where the dense call misses them."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, "tests"), os.path.join(ROOT, "scripts")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import box_pairs_host as H  # noqa: E402
from test_batch_contract_gpu import switches  # noqa: E402

pytestmark = pytest.mark.gpu

ABS_TOL = 1e-7
# pairs (i, j), i > j, on which the DENSE call differs from the reference's is_adjacent, per family of the fixture: the
# sparse call may differ from the fixture there and nowhere else
DENSE_DIFFERS = {"a": [], "b": [], "c": [], "d": []}


@pytest.fixture(scope="module")
def env():
    import torch
    import polytope_amd as pa
    from polytope_amd import solvers
    assert torch.cuda.is_available()
    saved, solvers.default_solver = solvers.default_solver, "hip"
    yield torch, pa, torch.device("cuda:0")
    solvers.default_solver = saved


@pytest.fixture(scope="module")
def L(tmp_path_factory):
    return H.build(tmp_path_factory.mktemp("box_pairs_host"))


@pytest.fixture(scope="module")
def fx():
    return H.load_fixture()


@pytest.fixture(scope="module")
def boxes():
    return {c[0]: c[1:] for c in H.box_cases()}


def _dev(torch, dev, *arrays):
    return [None if a is None else torch.as_tensor(np.ascontiguousarray(a)).to(dev) for a in arrays]


def _host(t):
    return t if isinstance(t, np.ndarray) else t.cpu().numpy()


def _check_sparse(env, A, b, m=None, n1=None, abs_tol=ABS_TOL, **kw):
    """sparse == dense for adjacency and overlap (and the cross form with n1) on CUDA tensors -> the adjacent pairs"""
    torch, pa, dev = env
    At, bt, mt = _dev(torch, dev, A, b, m)
    n = A.shape[0]
    adj = pa.adjacent_pairs_sparse(At, bt, m=mt, abs_tol=abs_tol, **kw)
    want = H.tril_pairs(_host(pa.adjacent_pairs(At, bt, m=mt, abs_tol=abs_tol))) if n else np.zeros((0, 2), np.int32)
    got = _host(adj["pairs"])
    assert got.dtype == np.int32 and got.shape == want.shape and np.array_equal(got, want)
    assert 0 <= adj["ncand"] <= n * (n - 1) // 2 and adj["ncand"] >= got.shape[0]
    ov = pa.overlap_pairs_sparse(At, bt, m=mt, abs_tol=abs_tol, **kw)
    want_ov = H.tril_pairs(_host(pa.batch.overlap_pairs(At, bt, m=mt, abs_tol=abs_tol))) if n else np.zeros((0, 2), np.int32)
    assert np.array_equal(_host(ov["pairs"]), want_ov)
    if n1:
        cr = pa.overlap_cross_sparse(At, bt, n1, m=mt, thresh=abs_tol, **kw)
        want_cr = np.argwhere(_host(pa.batch.overlap_cross(At, bt, n1, m=mt, thresh=abs_tol))).astype(np.int32)
        assert np.array_equal(_host(cr["pairs"]), want_cr)
    return got, adj["ncand"]


# ------------------------------------------------------------------------------------------------ the fixture's families
@pytest.mark.parametrize("name", ["a", "b", "c", "d"])
def test_fixture_families(env, fx, name):
    f = fx[name]
    n = f["A"].shape[0]
    got, ncand = _check_sparse(env, f["A"], f["b"], f["m"], n1=n // 3)
    want = H.tril_pairs(f["adj"])
    torch, pa, dev = env
    At, bt, mt = _dev(torch, dev, f["A"], f["b"], f["m"])
    dense = H.tril_pairs(_host(pa.adjacent_pairs(At, bt, m=mt, abs_tol=ABS_TOL)))

    def sym_diff(x, y):
        cx, cy = (set(map(tuple, v.tolist())) for v in (x, y))
        return sorted(cx ^ cy)
    print("family %s: %d cells, %d candidates, %d adjacent; dense differs from the reference on %s"
          % (name, n, ncand, got.shape[0], sym_diff(dense, want)))
    assert sym_diff(dense, want) == [tuple(p) for p in DENSE_DIFFERS[name]]
    assert set(sym_diff(got, want)) <= set(sym_diff(dense, want))
    if name in "ab":
        assert ncand < n * (n - 1) // 2
    if name == "a":
        assert ncand == 468 and got.shape[0] == 468


def test_gap_verdicts(env, fx):
    """family (d): the pairs 0, 1e-8 and 1.7e-7 apart are adjacent (the inflated cells overlap by more than 2e-8), those
    1.9e-7, 2.1e-7 and 1e-6 apart are not; the sparse call says so"""
    f = fx["d"]
    got, _ = _check_sparse(env, f["A"], f["b"])
    assert got.tolist() == [[1, 0], [3, 2], [5, 4]]


# ------------------------------------------------------------------------------------------------ the broad phase
@pytest.mark.parametrize("name", H.box_case_names())
def test_device_broad_phase_is_the_host_brute_force(env, L, boxes, name):
    torch, pa, dev = env
    lb, ub = boxes[name]
    n = lb.shape[0]
    lbt, ubt = _dev(torch, dev, lb, ub)
    for n1 in (None, n // 3 if n >= 3 else None):
        per_cell, pairs = H.brute(L, lb, ub, n1 or 0)
        for grid in (None, "grid"):
            for walk in ({}, {"PLP_BOX_WALK": "1"}, {"PLP_BOX_WALK": "0"}):
                if grid is None and walk:
                    continue
                with switches(walk):
                    got = pa.box_pairs(lbt, ubt, n1=n1, grid=grid)
                    what = (name, n1, grid, walk)
                    assert got["ncand"] == pairs.shape[0], what
                    assert np.array_equal(_host(got["per_cell"]), per_cell), what
                    assert np.array_equal(_host(got["pairs"]), pairs), what
                    if name in ("slab", "big_box", "grid3_4096", "halfspace") and grid == "grid":
                        assert got["grid"] is not None, what     # (the walk under test really ran over lists)
        # numpy in, numpy out: the host-pointer entry points
        got = pa.box_pairs(lb, ub, n1=n1, grid="grid")
        assert isinstance(got["pairs"], np.ndarray) and np.array_equal(got["pairs"], pairs)
        assert np.array_equal(got["per_cell"], per_cell)


def test_fill_by_cell_range(env, L, boxes):
    """the pairs of a range of cells are the slice of the whole list"""
    torch, pa, dev = env
    from polytope_amd import batch
    lb, ub = boxes["big_box"]
    _, pairs = H.brute(L, lb, ub)
    for src in (_dev(torch, dev, lb, ub), (lb, ub)):
        for walk in ("0", "1"):
            with switches({"PLP_BOX_WALK": walk}):
                bp = batch._BoxPairs(batch._Backend(src[0]), src[0], src[1], None, batch._LOCATE_PAD, "grid")
                pc = _host(bp.per_cell)
                for lo, hi in ((0, 1), (1, 50), (50, 102), (101, 102), (7, 7)):
                    assert np.array_equal(_host(bp.fill(lo, hi)), pairs[pc[lo]:pc[hi]]), (walk, lo, hi)


# ------------------------------------------------------------------------------------------------ listed pairs
def _all_pairs_shuffled(n, rng):
    ii, jj = np.tril_indices(n, -1)
    p = np.stack([ii, jj], 1).astype(np.int32)
    flip = rng.random(p.shape[0]) < 0.5
    p[flip] = p[flip][:, ::-1]
    return p[rng.permutation(p.shape[0])]


LISTED = [
    # (name, grid shape, PLP_ADJ_WIDE or None): the engine the list gets is plan_pair_list's, sized by K
    ("d1", (10,), None),
    ("d2", (5, 4), None),
    ("d3", (4, 4, 4), None),
    ("d4", (3, 3, 2, 2), None),
    ("d6_few", (3, 3, 2, 2, 1, 1), None),        # 630 pairs <= 4096: one pair per wavefront
    ("d6_many", (3, 3, 3, 2, 2, 1), None),       # 5778 pairs > 4096: lane groups
    ("d6_many_wide", (3, 3, 3, 2, 2, 1), "1"),
    ("d6_few_group", (3, 3, 2, 2, 1, 1), "0"),
    ("d9", (3, 3, 2, 1, 1, 1, 1, 1, 1), None),
]


@pytest.mark.parametrize("name,shape,wide", LISTED, ids=[c[0] for c in LISTED])
def test_pair_verdicts_are_the_dense_entries(env, name, shape, wide):
    torch, pa, dev = env
    rng = np.random.default_rng(5)
    A, b, _ = H.grid_cells(shape)
    b = b + 0.05 * rng.random(b.shape)          # cells overlap a little: overlap verdicts of both kinds
    n = A.shape[0]
    At, bt = _dev(torch, dev, A, b)
    pairs = _all_pairs_shuffled(n, rng)
    pt, = _dev(torch, dev, pairs)
    with switches({} if wide is None else {"PLP_ADJ_WIDE": wide}):
        for inflate, thresh, dense_fn in ((ABS_TOL, ABS_TOL / 10, pa.adjacent_pairs), (0.0, ABS_TOL, pa.batch.overlap_pairs)):
            D = _host(dense_fn(At, bt, abs_tol=ABS_TOL))
            v = _host(pa.pair_verdicts(At, bt, pt, inflate=inflate, thresh=thresh))
            assert v.dtype == np.uint8 and np.array_equal(v, D[pairs[:, 0], pairs[:, 1]]), name
            assert 0 < v.sum() < v.size
        # the sparse call on the same cells: a list of fewer pairs may go to the other engine than the dense call's
        _check_sparse(env, A, b)
    # numpy in, numpy out
    v = pa.pair_verdicts(A, b, pairs[:200], inflate=ABS_TOL, thresh=ABS_TOL / 10)
    assert np.array_equal(v, _host(pa.adjacent_pairs(At, bt, abs_tol=ABS_TOL))[pairs[:200, 0], pairs[:200, 1]])


def test_d5_more_than_4096_candidates(env):
    """the 3^5 grid: 8282 touching pairs, so the listed engine is the lane groups' as the dense call's"""
    A, b, idx = H.grid_cells((3, 3, 3, 3, 3))
    got, ncand = _check_sparse(env, A, b)
    assert ncand == 8282 and np.array_equal(got, H.grid_touching(idx))


def test_bad_pairs(env):
    torch, pa, dev = env
    A, b, _ = H.grid_cells((3, 3))
    pairs = np.array([[1, 0], [9, 0], [0, -1], [4, 4], [8, 7], [2, 5]], np.int32)
    with pytest.raises(ValueError):
        pa.pair_verdicts(A, b, pairs)
    At, bt, pt = _dev(torch, dev, A, b, pairs)
    for d6 in (False, True):    # both engines
        if d6:
            A6, b6, _ = H.grid_cells((3, 3, 1, 1, 1, 1))
            At, bt = _dev(torch, dev, A6, b6)
        v = _host(pa.pair_verdicts(At, bt, pt, inflate=ABS_TOL, thresh=ABS_TOL / 10))
        D = _host(pa.adjacent_pairs(At, bt, abs_tol=ABS_TOL))
        assert v.tolist() == [D[1, 0], 255, 255, 255, D[8, 7], D[2, 5]]


# ------------------------------------------------------------------------------------------------ special families
def _cells_of(lb, ub):
    A, b = H.box_cells(np.where(np.isfinite(lb), lb, -50.0), np.where(np.isfinite(ub), ub, 50.0))
    return A, b


def test_small_tables(env, boxes):
    for n in (1, 2):
        A, b, _ = H.grid_cells((n, 1))
        got, ncand = _check_sparse(env, A, b, n1=1 if n == 2 else None)
        assert got.shape[0] == n - 1


def test_slab_and_big_box(env, boxes):
    for name in ("slab", "big_box"):
        for walk in ("0", "1"):
            with switches({"PLP_BOX_WALK": walk}):
                A, b = _cells_of(*boxes[name])
                got, ncand = _check_sparse(env, A, b, n1=A.shape[0] // 2)
                assert got.shape[0] > 64


def test_halfspace_infeasible_rowless_ragged(env):
    rng = np.random.default_rng(8)
    A0, b0, _ = H.grid_cells((6, 5))
    n = A0.shape[0]
    A = np.concatenate([A0, rng.standard_normal((n, 2, 2))], 1)       # two spare rows per cell
    b = np.concatenate([b0, np.full((n, 2), 100.0)], 1)
    m = rng.integers(4, 7, n).astype(np.int32)
    m[7] = 1                       # a half-space: x0 <= b (its box is infinite)
    m[12] = 0                      # no rows: the whole space
    A[20, 4], b[20, 4], m[20] = [1.0, 0.0], -100.0, 5      # infeasible: x0 <= -100 against x0 >= its lower side
    A[25, 4], b[25, 4], m[25] = [0.0, 0.0], 1.0, 5         # a zero row
    got, ncand = _check_sparse(env, A, b, m, n1=10)
    assert (got == 7).any() and (got == 12).any() and not (got == 20).any()
    # nothing is read past m[p]: NaN in the rows beyond changes nothing
    A2, b2 = A.copy(), b.copy()
    for p in range(n):
        A2[p, m[p]:], b2[p, m[p]:] = np.nan, np.nan
    got2, ncand2 = _check_sparse(env, A2, b2, m, n1=10)
    assert np.array_equal(got2, got) and ncand2 == ncand


def test_no_candidates_and_many_chunks(env, L):
    torch, pa, dev = env
    A, b, _ = H.grid_cells((5, 5), width=1.0)
    b[:, :2] -= 0.5                                     # cells of width 0.5, a gap of 0.5 between neighbours
    got, ncand = _check_sparse(env, A, b, n1=10)
    assert ncand == 0 and got.shape == (0, 2)
    A, b, idx = H.grid_cells((6, 6, 3))
    whole, ncand = _check_sparse(env, A, b, n1=30)
    for cap in (64, 1, 7):
        chunked, nc = _check_sparse(env, A, b, n1=30, max_candidates=cap)
        assert np.array_equal(chunked, whole) and nc == ncand
    # numpy == torch, boxes passed in == boxes computed, two runs give identical bytes
    lbx, ubx = H.exact_boxes(A, b, None, ABS_TOL)
    r_np = pa.adjacent_pairs_sparse(A, b, max_candidates=64)
    r_bx = pa.adjacent_pairs_sparse(A, b, boxes=(lbx, ubx))
    assert isinstance(r_np["pairs"], np.ndarray) and np.array_equal(r_np["pairs"], whole)
    assert np.array_equal(r_bx["pairs"], whole) and r_bx["ncand"] == ncand
    At, bt = _dev(torch, dev, A, b)
    r1, r2 = pa.adjacent_pairs_sparse(At, bt), pa.adjacent_pairs_sparse(At, bt)
    assert r1["pairs"].is_cuda and torch.equal(r1["pairs"], r2["pairs"]) and r1["ncand"] == r2["ncand"]


CAREFUL = ("pairs-adjacent_r_kernel<8,8>-B28-m16-ADJ_WIDE=0", "pairs-adjacent_w_kernel<15>-B28-m32-default")


@pytest.mark.parametrize("cid", CAREFUL)
def test_pairs_that_end_in_the_careful_pass(env, cid):
    """the cases of tests/instance_cases.py whose pairs the engines leave open (a `dup` cell stacked on a `ragged` one: the
    careful pass decides): the listed engines mark the same pairs, and the same pass decides them"""
    import instance_cases as ic
    torch, pa, dev = env
    case = [c for c in ic.CASES if ic.case_id(c) == cid]
    assert len(case) == 1
    call, B, m_max, d, sw = case[0][:5]
    mem = ic.members(case[0])
    At, bt, mt = _dev(torch, dev, mem["A"], mem["b"], mem["m"])
    rng = np.random.default_rng(3)
    pairs = _all_pairs_shuffled(B, rng)
    pt, = _dev(torch, dev, pairs)
    with switches(sw):
        for inflate, thresh, dense_fn in ((ABS_TOL, ABS_TOL / 10, pa.adjacent_pairs), (0.0, ABS_TOL, pa.batch.overlap_pairs)):
            D = _host(dense_fn(At, bt, m=mt, abs_tol=ABS_TOL))
            v = _host(pa.pair_verdicts(At, bt, pt, m=mt, inflate=inflate, thresh=thresh))
            assert v.max() <= 1 and np.array_equal(v, D[pairs[:, 0], pairs[:, 1]])
        _check_sparse(env, mem["A"], mem["b"], mem["m"], n1=9)


# ------------------------------------------------------------------------------------------------ the object layer
def test_adjacency_sparse_objects(env, fx):
    torch, pa, dev = env
    import scipy.sparse as sp
    from polytope_amd import polytope as pc, prop2partition as p2p, _lib
    f = fx["a"]
    cells = [pc.Polytope(A, b, normalize=False) for A, b in zip(f["A"], f["b"])]
    part = [pc.Region([c]) for c in cells]
    got = p2p.adjacency_sparse(part)
    want = p2p.find_adjacent_regions(part).tocsr()
    assert sp.isspmatrix_csr(got) and got.dtype == np.int8 and got.shape == (64, 64)
    assert (got != want).nnz == 0 and np.array_equal(got.toarray(), f["adj"].astype(np.int8))
    # Regions of two members: folded by `any`
    two = [pc.Region([cells[2 * k], cells[2 * k + 1]]) for k in range(32)]
    got2, want2 = p2p.adjacency_sparse(two), p2p.find_adjacent_regions(two).tocsr()
    assert got2.shape == (32, 32) and (got2 != want2).nnz == 0 and np.array_equal(got2.toarray(), want2.toarray())
    ov = p2p.overlap_sparse(two)
    assert np.array_equal(ov.toarray() != 0, p2p.overlap_matrix_dense(two))
    big = pc.Polytope(np.vstack([np.eye(3)] * 11), np.ones(33), normalize=False)
    with pytest.raises(_lib.UnsupportedSize):
        p2p.adjacency_sparse([pc.Region([big]), pc.Region([cells[0]])])
