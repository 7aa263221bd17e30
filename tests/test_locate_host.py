"""CPU: point location (polytope_amd/csrc/plp_locate.hpp built with g++ -ffp-contract=off, tests/locate_host.py) -- the
sequential dense answer against the reference's (tests/golden/locate.npz), the grid answer against the dense one on every
case family of the GPU tests, the properties the cull rests on (monotone cell map, ranges that cover, ascending lists),
and what of locate_batch / Region.locate / Partition.locate needs no device."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import locate_host as LH  # noqa: E402
from conftest import load_golden  # noqa: E402

SETS = ("a", "b", "c")


@pytest.fixture(scope="module")
def L(tmp_path_factory):
    return LH.build(tmp_path_factory.mktemp("locate_host"))


@pytest.fixture(scope="module")
def gold():
    return load_golden("locate.npz")


@pytest.fixture(scope="module")
def cases():
    return LH.cases()


@pytest.fixture(scope="module")
def grids(L, oracle, cases, gold):
    """name -> (A, b, m, X, tol, host grid) for the case families and the three fixture sets; built once"""
    out = {}
    for name, A, b, m, X, tol in cases:
        out[name] = (A, b, m, X, tol, LH.host_grid(L, oracle, A, b, m, tol))
    for s in SETS:
        A, b, m, X = (gold["%s_%s" % (s, k)] for k in ("A", "b", "m", "X"))
        out["gold_" + s] = (A, b, m, X, 1e-7, LH.host_grid(L, oracle, A, b, m, 1e-7))
    return out


def test_package_root_exports():
    import polytope_amd as pa
    from polytope_amd import batch
    assert pa.locate_batch is batch.locate_batch and pa.locate_grid is batch.locate_grid
    assert callable(pa.Region.locate) and callable(pa.Partition.locate)


@pytest.mark.parametrize("s", SETS)
def test_host_dense_equals_reference(L, gold, s):
    first, count = LH.locate(L, gold[s + "_A"], gold[s + "_b"], gold[s + "_X"], 1e-7, m=gold[s + "_m"])
    assert np.array_equal(first, gold[s + "_first_member"])
    assert np.array_equal(count, gold[s + "_count_member"])
    region = gold[s + "_region"]
    assert np.array_equal(np.where(first >= 0, region[np.maximum(first, 0)], -1), gold[s + "_first_region"])


def test_host_grid_equals_host_dense(L, grids):
    used = 0
    for name, (A, b, m, X, tol, g) in grids.items():
        fd, cd = LH.locate(L, A, b, X, tol, m=m)
        fg, cg = LH.locate(L, A, b, X, tol, m=m, grid=g)
        assert np.array_equal(fd, fg) and np.array_equal(cd, cg), name
        used += g.kind == "grid"
    assert used >= len(grids) // 2   # (the families are not all declined: the grid path is what ran)


def test_fixture_sets_get_a_grid(grids):
    for s in SETS[:2]:   # the two partitions separate along every axis
        g = grids["gold_" + s][5]
        assert g.kind == "grid" and g.cells > 1 and g.max_list < g.shape[0]


def test_cell_map_is_monotone(L):
    rng = np.random.default_rng(7)
    lo, res = -1.0, 37
    inv_h = res / 2.0
    edges = lo + np.arange(res + 1) / inv_h
    x = np.concatenate([
        rng.uniform(-3, 3, 100000 - 8 * (res + 1) - 16), edges, np.nextafter(edges, -np.inf), np.nextafter(edges, np.inf),
        edges + 1e-12, edges - 1e-12, edges * (1 + 1e-15), edges * (1 - 1e-15), edges + 0.0,
        [np.inf, -np.inf, 0.0, -0.0, 5e-324, -5e-324, 2.2e-308, -2.2e-308, 1e-310, -1e-310, 1e300, -1e300, 1.0, -1.0, 3.0, -3.0]])
    x.sort()
    assert x.size == 100000
    for args in ((lo, inv_h, res), (lo, 0.0, 1), (0.0, 1e300, 4096), (-1e-310, 1e-3, 5), (lo, inv_h, 1)):
        c = LH.cells(L, x, *args)
        assert c.min() >= 0 and c.max() <= args[2] - 1
        assert np.all(np.diff(c) >= 0), args
    c = LH.cells(L, x, lo, inv_h, res)
    assert c[0] == 0 and c[-1] == res - 1 and set(c.tolist()) == set(range(res))
    assert LH.cells(L, np.array([np.nan]), lo, inv_h, res)[0] == 0


def test_ranges_cover_every_accepted_point(L, grids):
    checked = 0
    for name, (A, b, m, X, tol, g) in grids.items():
        if g.kind != "grid" or X.shape[1] == 0:
            continue
        listed, c_lo, c_hi = LH.cell_ranges(L, g.desc, g.lb, g.ub)
        na = g.desc.naxes
        cell = np.stack([LH.cells(L, X[g.desc.axis[j]], g.desc.lo[j], g.desc.inv_h[j], g.desc.res[j]) for j in range(na)], 1)
        for p in range(A.shape[0]):
            mp = A.shape[1] if m is None else int(m[p])
            f, _ = LH.locate(L, A[p:p + 1, :max(mp, 0)], b[p:p + 1, :max(mp, 0)], X, tol) if mp else (np.zeros(X.shape[1], np.int32), None)
            inside = f == 0
            if not inside.any():
                continue
            assert listed[p], (name, p)
            assert np.all((cell[inside] >= c_lo[p, :na]) & (cell[inside] <= c_hi[p, :na])), (name, p)
            checked += int(inside.sum())
    assert checked > 1000


def test_cell_items_ascending_and_consistent(L, grids):
    for name, (A, b, m, X, tol, g) in grids.items():
        if g.kind != "grid":
            continue
        cs, it = g.cell_start, g.cell_items
        assert cs[0] == 0 and np.all(np.diff(cs) >= 0) and cs[-1] == it.size == g.n_items, name
        assert it.size == 0 or (it.min() >= 0 and it.max() < A.shape[0]), name
        inner = np.ones(it.size, bool)
        inner[cs[:-1][cs[:-1] < it.size]] = False          # first entry of every non-empty list
        assert np.all(np.diff(it)[inner[1:]] > 0), name     # strictly ascending inside a list
        assert g.max_list == np.diff(cs).max(), name


def test_declined_grids_report_dense(L, oracle, grids):
    for name in ("all_span", "list_cap", "P0"):
        assert grids[name][5].kind == "dense", name
    A, b, m, X, tol, g = grids["gold_a"]
    assert g.kind == "grid"
    assert LH.host_grid(L, oracle, A, b, m, tol, max_items=g.n_items - 1).kind == "dense"
    assert LH.host_grid(L, oracle, A, b, m, tol, max_list=g.max_list - 1).kind == "dense"


def test_locate_batch_arguments_without_a_device():
    import polytope_amd as pa
    from polytope_amd.batch import LocateGrid
    A, b = np.zeros((3, 4, 2)), np.zeros((3, 4))
    with pytest.raises(ValueError, match="column vectors"):
        pa.locate_batch(A, b, np.zeros((3, 5)))
    with pytest.raises(ValueError, match="column vectors"):
        pa.locate_batch(A, b, np.zeros(2))
    with pytest.raises(ValueError):
        pa.locate_batch(np.zeros((3, 4)), b, np.zeros((2, 5)))
    with pytest.raises(ValueError, match="grid must be"):
        pa.locate_batch(A, b, np.zeros((2, 5)), grid="dense")
    with pytest.raises(ValueError, match="abs_tol"):
        pa.locate_batch(A, b, np.zeros((2, 5)), abs_tol=1e-7, grid=LocateGrid("dense", 1e-6, (3, 4, 2)))
    with pytest.raises(ValueError, match="shape"):
        pa.locate_batch(A, b, np.zeros((2, 5)), grid=LocateGrid("dense", 1e-7, (4, 4, 2)))
    # N = 0 returns before the library is touched
    first = pa.locate_batch(A, b, np.zeros((2, 0)))
    assert first.shape == (0,) and first.dtype == np.int32
    first, count = pa.locate_batch(A, b, np.zeros((2, 0)), count=True, grid=LocateGrid("dense", 1e-7, (3, 4, 2)))
    assert first.shape == count.shape == (0,) and count.dtype == np.int32


def test_more_than_64_rows_decline_without_a_device():
    """bbox_batch takes up to 64 rows; the dense kernel any number: such a table gets a declined grid, before any library call"""
    import polytope_amd as pa
    g = pa.locate_grid(np.zeros((600, 65, 2)), np.zeros((600, 65)))
    assert g.kind == "dense" and g.shape == (600, 65, 2) and "64" in g.reason
    g = pa.locate_grid(np.zeros((3, 200, 4)), np.zeros((3, 200)), m=np.array([1, 2, 3], np.int32), abs_tol=1e-6)
    assert g.kind == "dense" and g.abs_tol == 1e-6


@pytest.fixture
def scipy_backend():
    from polytope_amd import solvers
    saved, solvers.default_solver = solvers.default_solver, "scipy"
    yield
    solvers.default_solver = saved


def _regions_of_set(pa, gold, s):
    A, b, m, region = (gold["%s_%s" % (s, k)] for k in ("A", "b", "m", "region"))
    regions = []
    for r in range(int(region.max()) + 1):
        regions.append(pa.Region([pa.Polytope(A[k, :m[k]].copy(), b[k, :m[k]].copy(), normalize=False)
                                  for k in np.nonzero(region == r)[0]]))
    return regions


@pytest.mark.parametrize("s", SETS)
def test_objects_on_the_numpy_backend(gold, scipy_backend, s):
    import polytope_amd as pa
    regions = _regions_of_set(pa, gold, s)
    X = gold[s + "_X"]
    part = pa.Partition()
    part.regions = regions
    got = part.locate(X)
    assert got.dtype == np.int32 and np.array_equal(got, gold[s + "_first_region"])
    # one Region of all members (an empty description in second place, which contains nothing): positions in list_poly
    members = [p for r in regions for p in r.list_poly]
    flat = pa.Region(members)
    flat.list_poly.insert(1, pa.Polytope())   # (the constructor drops empty members; one put there afterwards stays)
    want = gold[s + "_first_member"]
    assert np.array_equal(flat.locate(X), np.where(want >= 1, want + 1, want))
    with pytest.raises(ValueError, match="column vectors"):
        flat.locate(np.zeros((X.shape[0] + 1, 3)))
