"""GPU: point location (csrc/plp_locate.hip through locate_batch / locate_grid / Region.locate / Partition.locate).
Device dense == device grid == the host restatement (tests/locate_host.py), as integer equality of `first` and `count`, on
the case families of locate_host.cases(); the fixture of the reference's answers; first == arg-max of contains_batch;
nothing read past m[p]; nothing written outside the outputs; numpy == torch; streams; determinism; resident tables."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import locate_host as LH  # noqa: E402
from conftest import load_golden  # noqa: E402

pytestmark = pytest.mark.gpu

NAMES = LH.case_names()      # (names only: the families are built by the `cases` fixture, not at collection)
SETS = ("a", "b", "c")


@pytest.fixture(scope="module")
def cases():
    return {c[0]: c for c in LH.cases()}


@pytest.fixture(scope="module")
def L(tmp_path_factory):
    return LH.build(tmp_path_factory.mktemp("locate_host"))


@pytest.fixture(scope="module")
def gold():
    return load_golden("locate.npz")


@pytest.fixture(scope="module")
def env():
    import torch
    import polytope_amd as pa
    from polytope_amd import solvers
    assert torch.cuda.is_available()
    saved, solvers.default_solver = solvers.default_solver, "hip"
    yield torch, pa, torch.device("cuda:0")
    solvers.default_solver = saved


def _dev(torch, dev, *arrays):
    return [None if a is None else torch.as_tensor(np.ascontiguousarray(a)).to(dev) for a in arrays]


def _three_ways(env, L, A, b, m, X, tol):
    """-> grid, [(first, count)] for device dense, device grid, host dense -- numpy int32"""
    torch, pa, dev = env
    At, bt, mt, Xt = _dev(torch, dev, A, b, m, X)
    g = pa.locate_grid(At, bt, mt, tol)
    out = []
    for grid in (None, g):
        f, c = pa.locate_batch(At, bt, Xt, tol, m=mt, count=True, grid=grid)
        f1 = pa.locate_batch(At, bt, Xt, tol, m=mt, grid=grid)       # the early-exit form
        assert f.dtype == torch.int32 and c.dtype == torch.int32 and torch.equal(f, f1)
        out.append((f.cpu().numpy(), c.cpu().numpy()))
    out.append(LH.locate(L, A, b, X, tol, m=m))
    return g, out


@pytest.mark.parametrize("name", NAMES)
def test_dense_grid_host_agree(env, L, cases, name):
    name, A, b, m, X, tol = cases[name]
    g, (dd, dg, hh) = _three_ways(env, L, A, b, m, X, tol)
    assert np.array_equal(dd[0], hh[0]) and np.array_equal(dd[1], hh[1]), name
    assert np.array_equal(dg[0], hh[0]) and np.array_equal(dg[1], hh[1]), (name, g)
    if name in ("all_span", "list_cap", "P0"):
        assert g.kind == "dense", g
    if name in ("overlap_dup", "outside_inf_nan", "halfspaces", "rescaled", "zero_rows", "ragged_m0_middle", "d2", "d3_N65"):
        assert g.kind == "grid", g          # (the cases written for the grid do run on it)
    if name == "overlap_dup":
        assert hh[1].max() > 1


def test_rescaled_probes_sit_in_the_relaxed_margin(cases):
    """the `rescaled` family holds points outside an unrelaxed facet of a 1e-6-scaled row that the dense test accepts"""
    name, A, b, m, X, tol = cases["rescaled"]
    s = np.einsum("pik,kn->pin", A, X) - b[:, :, None]
    inside_relaxed = np.all(s < tol, axis=1)
    inside_strict = np.all(s <= 0, axis=1)
    assert int((inside_relaxed & ~inside_strict).sum()) >= 20


@pytest.mark.parametrize("s", SETS)
def test_fixture(env, gold, s):
    torch, pa, dev = env
    A, b, m, X, region = (gold["%s_%s" % (s, k)] for k in ("A", "b", "m", "X", "region"))
    At, bt, mt, Xt = _dev(torch, dev, A, b, m, X)
    for grid in (None, pa.locate_grid(At, bt, mt)):
        f, c = pa.locate_batch(At, bt, Xt, m=mt, count=True, grid=grid)
        assert np.array_equal(f.cpu().numpy(), gold[s + "_first_member"])
        assert np.array_equal(c.cpu().numpy(), gold[s + "_count_member"])
    regions = [pa.Region([pa.Polytope(A[k, :m[k]].copy(), b[k, :m[k]].copy(), normalize=False) for k in np.nonzero(region == r)[0]])
               for r in range(int(region.max()) + 1)]
    part = pa.Partition()
    part.regions = regions
    assert np.array_equal(part.locate(X), gold[s + "_first_region"])
    flat = pa.Region([p for r in regions for p in r.list_poly])
    flat.list_poly.insert(1, pa.Polytope())
    want = gold[s + "_first_member"]
    assert np.array_equal(flat.locate(X), np.where(want >= 1, want + 1, want))


def _overlapping(P, N, d=3, seed=5):
    from polytope_amd.synth import containment_workload
    A, b, X = containment_workload(P, N, d=d, m=12, seed=seed)
    return A, b, np.ascontiguousarray(X * 0.8)


def test_first_is_argmax_of_contains(env):
    torch, pa, dev = env
    A, b, X = _overlapping(40, 5000)
    m = np.random.default_rng(1).integers(6, 13, 40).astype(np.int32)
    At, bt, mt, Xt = _dev(torch, dev, A, b, m, X)
    M = pa.contains_batch(At, bt, Xt, m=mt, region=False).to(torch.int32)
    any_ = M.sum(0) > 0
    want_first = torch.where(any_, M.argmax(0).to(torch.int32), torch.full_like(M[0], -1))
    assert int(any_.sum()) > 500 and int((M.sum(0) > 1).sum()) > 100
    for grid in (None, pa.locate_grid(At, bt, mt)):
        f, c = pa.locate_batch(At, bt, Xt, m=mt, count=True, grid=grid)
        assert torch.equal(f, want_first) and torch.equal(c, M.sum(0).to(torch.int32))


@pytest.mark.parametrize("kind", ["nan", "exclude"])
def test_rows_past_m_are_not_read(env, kind):
    torch, pa, dev = env
    A, b, X = _overlapping(30, 1000, seed=6)
    m = np.random.default_rng(2).integers(0, 13, 30).astype(np.int32)
    m[[0, 7, 29]] = [0, 12, 0]
    A2, b2 = A.copy(), b.copy()
    dead = np.arange(12)[None, :] >= m[:, None]
    if kind == "nan":
        A2[dead], b2[dead] = np.nan, np.nan
    else:
        A2[dead], b2[dead] = 0.0, -1.0       # 0 . x - (-1) < tol is false: such a row, if read, excludes every point
    At, bt, mt, Xt, A2t, b2t = _dev(torch, dev, A, b, m, X, A2, b2)
    for build in (lambda a, bb: None, lambda a, bb: pa.locate_grid(a, bb, mt)):
        f0, c0 = pa.locate_batch(At, bt, Xt, m=mt, count=True, grid=build(At, bt))
        g1 = build(A2t, b2t)
        f1, c1 = pa.locate_batch(A2t, b2t, Xt, m=mt, count=True, grid=g1)
        assert torch.equal(f0, f1) and torch.equal(c0, c1)
        assert int(c0.min()) >= 2          # (the two rowless polytopes contain every point)


def test_outputs_stay_inside_their_slices(env):
    torch, pa, dev = env
    from polytope_amd import _lib
    from polytope_amd.batch import _torch_stream_ctx
    A, b, X = _overlapping(20, 777, seed=8)
    At, bt, Xt = _dev(torch, dev, A, b, X)
    N, pad = 777, 300
    g = pa.locate_grid(At, bt)
    assert g.kind == "grid"
    want_f, want_c = pa.locate_batch(At, bt, Xt, count=True, grid=None)
    lib = _lib.load()
    _, ctx, stream = _torch_stream_ctx(Xt)
    for grid in (None, g):
        for with_count in (True, False):
            big_f = torch.full((N + 2 * pad,), -77, dtype=torch.int32, device=dev)
            big_c = torch.full((N + 2 * pad,), -88, dtype=torch.int32, device=dev)
            pf, pc = big_f.data_ptr() + 4 * pad, big_c.data_ptr() + 4 * pad
            rc = lib.plp_locate_dev(ctx.handle, stream, 20, 12, 3, At.data_ptr(), bt.data_ptr(), None, N, Xt.data_ptr(), 1e-7,
                                    None if grid is None else C.addressof(grid.desc),
                                    None if grid is None else grid.cell_start.data_ptr(),
                                    None if grid is None else grid.cell_items.data_ptr(), pf, pc if with_count else None)
            assert rc == 0
            assert torch.equal(big_f[pad:pad + N], want_f)
            assert bool((big_f[:pad] == -77).all()) and bool((big_f[pad + N:] == -77).all())
            if with_count:
                assert torch.equal(big_c[pad:pad + N], want_c)
                assert bool((big_c[:pad] == -88).all()) and bool((big_c[pad + N:] == -88).all())
            else:
                assert bool((big_c == -88).all())


def test_numpy_and_torch_agree(env):
    torch, pa, dev = env
    A, b, X = _overlapping(25, 900, seed=9)
    m = np.random.default_rng(3).integers(3, 13, 25).astype(np.int32)
    At, bt, mt, Xt = _dev(torch, dev, A, b, m, X)
    gt, gn = pa.locate_grid(At, bt, mt), pa.locate_grid(A, b, m)
    assert gt.kind == gn.kind == "grid" and isinstance(gn.cell_items, np.ndarray)
    assert gt.axes == gn.axes and gt.res == gn.res
    assert np.array_equal(gt.cell_start.cpu().numpy(), gn.cell_start) and np.array_equal(gt.cell_items.cpu().numpy(), gn.cell_items)
    for grid_t, grid_n in ((None, None), (gt, gn), ("auto", "auto")):
        ft, ct = pa.locate_batch(At, bt, Xt, m=mt, count=True, grid=grid_t)
        fn, cn = pa.locate_batch(A, b, X, m=m, count=True, grid=grid_n)
        assert isinstance(fn, np.ndarray) and fn.dtype == np.int32
        assert np.array_equal(ft.cpu().numpy(), fn) and np.array_equal(ct.cpu().numpy(), cn)
    with pytest.raises(ValueError, match="both"):
        pa.locate_batch(A, b, X, m=m, grid=gt)
    # P = 0 through both entry points: first = -1, count = 0
    f, c = pa.locate_batch(A[:0], b[:0], X, count=True)
    assert np.all(f == -1) and np.all(c == 0)
    f, c = pa.locate_batch(At[:0], bt[:0], Xt, count=True)
    assert bool((f == -1).all()) and bool((c == 0).all())


def test_auto_builds_a_grid_for_1024_polytopes(env, L, monkeypatch):
    torch, pa, dev = env
    from polytope_amd import batch
    assert 64 < batch._LOCATE_AUTO_P <= 1024
    rng = np.random.default_rng(12)
    A, b = LH._cells_table(2, 32, rng)
    X = LH._points(rng, 2, 3000, 1.2)
    At, bt, Xt = _dev(torch, dev, A, b, X)
    built = []
    real = batch.locate_grid

    def counting(*args, **kw):
        built.append(real(*args, **kw))
        return built[-1]
    monkeypatch.setattr(batch, "locate_grid", counting)
    f, c = pa.locate_batch(At, bt, Xt, count=True)           # grid="auto", P = 1024
    assert len(built) == 1 and built[0].kind == "grid" and built[0].max_list <= 16     # the path taken, not only the answer
    pa.locate_batch(At[:64], bt[:64], Xt)                    # P = 64: dense, nothing built
    pa.locate_batch(At, bt, Xt, grid=None)
    assert len(built) == 1
    hf, hc = LH.locate(L, A, b, X)
    assert np.array_equal(f.cpu().numpy(), hf) and np.array_equal(c.cpu().numpy(), hc)


def test_more_than_64_rows_run_dense(env, L):
    """bbox_batch boxes up to 64 rows; the dense kernel has no row limit: the grid is declined, nothing raises"""
    torch, pa, dev = env
    from polytope_amd import batch
    rng = np.random.default_rng(15)
    A, b = LH._cells_table(2, 25, rng)                      # 625 cells >= the switch point of "auto"
    assert A.shape[0] >= batch._LOCATE_AUTO_P
    extra = rng.standard_normal((625, 61, 2))
    cen = np.stack([(b[:, 0] - b[:, 2]) / 2, (b[:, 1] - b[:, 3]) / 2], 1)
    A = np.concatenate([A, extra], 1)                       # m_max = 65: 61 tilted rows around each cell
    b = np.concatenate([b, np.einsum("pik,pk->pi", extra, cen) + 0.05 * np.linalg.norm(extra, axis=2)], 1)
    assert A.shape[1] == 65
    X = LH._points(rng, 2, 2000, 1.1)
    At, bt, Xt = _dev(torch, dev, A, b, X)
    assert pa.locate_grid(At, bt).kind == "dense"
    fa, ca = pa.locate_batch(At, bt, Xt, count=True)         # grid="auto"
    fd, cd = pa.locate_batch(At, bt, Xt, count=True, grid=None)
    hf, hc = LH.locate(L, A, b, X)
    assert torch.equal(fa, fd) and torch.equal(ca, cd)
    assert np.array_equal(fd.cpu().numpy(), hf) and np.array_equal(cd.cpu().numpy(), hc) and (hf >= 0).sum() > 200
    polys = [pa.Polytope(A[k].copy(), b[k].copy(), normalize=False) for k in range(625)]
    part = pa.Partition()
    part.regions = polys
    assert np.array_equal(part.locate(X), hf)


def test_non_default_stream(env):
    torch, pa, dev = env
    A, b, X = _overlapping(20, 2000, seed=10)
    At, bt, Xt = _dev(torch, dev, A, b, X)
    want = pa.locate_batch(At, bt, Xt, count=True, grid=None)
    torch.cuda.synchronize()
    st = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(st):
        g = pa.locate_grid(At, bt)
        got_g = pa.locate_batch(At, bt, Xt, count=True, grid=g)
        got_d = pa.locate_batch(At, bt, Xt, count=True, grid=None)
    st.synchronize()
    for got in (got_g, got_d):
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])


def test_two_calls_are_identical(env):
    torch, pa, dev = env
    rng = np.random.default_rng(13)
    A, b = LH._cells_table(3, 5, rng, jitter=0.4)          # overlapping cells: lists of several entries, filled by atomics
    X = LH._points(rng, 3, 2000, 1.2)
    At, bt, Xt = _dev(torch, dev, A, b, X)
    g1, g2 = pa.locate_grid(At, bt), pa.locate_grid(At, bt)
    assert g1.kind == "grid" and g1.max_list > 1
    assert torch.equal(g1.cell_start, g2.cell_start) and torch.equal(g1.cell_items, g2.cell_items)
    r1, r2 = pa.locate_batch(At, bt, Xt, count=True, grid=g1), pa.locate_batch(At, bt, Xt, count=True, grid=g2)
    assert torch.equal(r1[0], r2[0]) and torch.equal(r1[1], r2[1])


def test_partition_keeps_table_and_grid(env):
    torch, pa, dev = env
    from polytope_amd import batch
    rng = np.random.default_rng(14)
    A, b = LH._cells_table(2, 32, rng)                      # 1024 cells: the objects build a grid
    polys = [pa.Polytope(A[k].copy(), b[k].copy(), normalize=False) for k in range(1024)]
    part = pa.Partition()
    part.regions = polys
    X = LH._points(rng, 2, 4000, 1.1)

    def loop(pp):
        first = np.full(X.shape[1], -1, np.int32)
        for k in range(len(pp) - 1, -1, -1):
            first[np.all(pp[k].A.dot(X) - pp[k].b[:, None] < 1e-7, axis=0)] = k
        return first
    r1 = part.locate(X)
    assert np.array_equal(r1, loop(polys))
    assert part.__dict__["_locate"][2].kind == "grid"
    assert part._packed[1] is part.__dict__["_locate"][0]          # the table lives on the partition, not only in the cache
    before = batch.h2d_bytes
    r2 = part.locate(X)
    assert batch.h2d_bytes - before == X.nbytes
    assert np.array_equal(r1, r2)
    grid_before = part.__dict__["_locate"][2]
    polys[17].b += 0.1                                      # in place: same arrays, new content
    before = batch.h2d_bytes
    r3 = part.locate(X)
    assert batch.h2d_bytes - before > X.nbytes
    assert part.__dict__["_locate"][2] is not grid_before
    assert np.array_equal(r3, loop(polys)) and not np.array_equal(r3, r1)
