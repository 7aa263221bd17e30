"""CPU (scipy backend): the Polytope-level intersect_pairs and the overlay of two partitions -- equal to the loop of
Polytope.intersect, and to the reference's results in tests/golden/intersect_pairs.npz -- and the argument errors of the new
packed calls that are raised before the library is touched."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import intersect_pairs_cases as IC  # noqa: E402


@pytest.fixture(scope="module")
def pa():
    import polytope_amd as pa
    old = pa.solvers.default_solver
    pa.solvers.default_solver = "scipy"
    yield pa
    pa.solvers.default_solver = old


@pytest.fixture(scope="module")
def fixture():
    return IC.load_fixture()


def _same(p, q):
    return p.A.shape == q.A.shape and np.array_equal(p.A, q.A) and np.array_equal(p.b, q.b) and p.minrep == q.minrep


@pytest.mark.parametrize("fam", ["b2", "b5", "b9", "c", "d"])
def test_intersect_pairs_equals_the_loop_and_the_fixture(pa, fixture, fam):
    f = fixture[fam]
    cells = IC.cells_of(pa, f)
    got = pa.intersect_pairs(cells, f["pairs"])
    want = [cells[i].intersect(cells[j]) for i, j in f["pairs"]]
    assert len(got) == len(want) == len(f["pairs"])
    for t, (g, w) in enumerate(zip(got, want)):
        assert _same(g, w), t
        assert IC.differs_from_fixture(f, t, g) is None, (t, IC.differs_from_fixture(f, t, g))


def test_intersect_pairs_special_operands(pa):
    a, b = pa.box2poly([[0, 1], [0, 1]]), pa.box2poly([[0.5, 2], [0.5, 2]])
    flat = pa.Polytope(np.array([[1.0, 0], [-1.0, 0], [0, 1.0], [0, -1.0]]), np.array([1.0, -1.0, 1.0, 0.0]))
    got = pa.intersect_pairs([a, b, flat, pa.Polytope()], [(0, 1), (0, 2), (3, 0), (0, 0), (1, 0)], abs_tol=1e-6)
    assert got[0].A.shape == (4, 2) and got[1].A.size == 0 and got[2].A.size == 0
    assert _same(got[3], a.intersect(a, 1e-6)) and got[4].A.shape == (4, 2)
    assert pa.intersect_pairs([a, b], []) == []
    with pytest.raises(Exception, match="defined only with other Polytope"):
        pa.intersect_pairs([a, "x"], [(0, 1)])
    with pytest.raises(Exception, match="different dimension"):
        pa.intersect_pairs([a, pa.box2poly([[0, 1]] * 3)], [(0, 1)])
    with pytest.raises(IndexError):
        pa.intersect_pairs([a, b], [(0, 2)])


def test_overlay_on_the_box_grids(pa, fixture):
    f = fixture["a"]
    cells = IC.cells_of(pa, f)
    first, second = cells[:18], [pa.Region([c]) for c in cells[18:]]   # (single-polytope Regions are taken as their member)
    got, parents = pa.overlay(first, second)
    live = np.nonzero(f["rm"] > 0)[0]
    want = np.stack([f["pairs"][live, 0], f["pairs"][live, 1] - 18], 1).astype(np.int32)
    assert parents.dtype == np.int32 and np.array_equal(parents, want) and len(got) == len(live) == 75
    for q, t in zip(got, live):
        assert IC.differs_from_fixture(f, int(t), q) is None, (t, IC.differs_from_fixture(f, int(t), q))


def test_overlay_arguments(pa):
    from polytope_amd._lib import UnsupportedSize
    a, b = pa.box2poly([[0, 1], [0, 1]]), pa.box2poly([[0.5, 2], [0.5, 2]])
    with pytest.raises(UnsupportedSize):
        pa.overlay([a], [pa.Region([a, b])])
    cells, parents = pa.overlay([], [a])
    assert cells == [] and parents.shape == (0, 2) and parents.dtype == np.int32
    part = pa.Partition()
    part.regions = [a, pa.box2poly([[5, 6], [5, 6]])]
    cells, parents = pa.overlay(part, [b])
    assert parents.tolist() == [[0, 0]] and cells[0].A.shape == (4, 2)


def test_packed_calls_argument_errors(pa):
    """Raised before anything of the library is called (no device here)."""
    from polytope_amd._lib import UnsupportedSize
    A, b = np.zeros((3, 4, 2)), np.zeros((3, 4))
    pairs = np.array([[0, 1]], np.int32)
    for fn in (pa.pair_stacks, pa.batch.intersect_pairs):
        with pytest.raises(ValueError, match=r"pairs must be \[K, 2\]"):
            fn(A, b, np.zeros((2, 3), np.int32))
        with pytest.raises(UnsupportedSize):
            fn(np.zeros((3, 33, 2)), np.zeros((3, 33)), pairs)
        with pytest.raises(UnsupportedSize):
            fn(np.zeros((3, 4, 17)), np.zeros((3, 4)), pairs)
        with pytest.raises(ValueError, match="inf, nan"):
            fn(np.full((3, 4, 2), np.nan), b, pairs)
    with pytest.raises(ValueError, match="n1 must lie"):
        pa.intersect_cross_sparse(A, b, 4)
    with pytest.raises(ValueError, match="max_candidates"):
        pa.intersect_cross_sparse(A, b, 1, max_candidates=0)
    with pytest.raises(UnsupportedSize):
        pa.intersect_cross_sparse(np.zeros((3, 33, 2)), np.zeros((3, 33)), 1)
    assert pa.batch.RF_BADPAIR == 64 and pa.batch.RF_BADPAIR & (1 | 2 | 4 | 8 | 16 | 32) == 0
