"""GPU: pair_dist_kernel<D, RV> (polytope_amd/csrc/plp_pair_dist.hip) behind batch.distance_pairs.

Raw device answers (resolve=False) equal the host build of the same source (tests/cabi/pair_dist_host.cpp) BIT FOR BIT --
dist, lb, x, y, status -- at every (D, RV) instance, with a tail tile at every RV, lists that cross a tile boundary, a bad
pair on the device-pointer form and on every soak family.  Resolved answers pass the duality proof of
tests/pair_dist_host.py (1e-9 E) and no status 1 is left.  Then the object-level calls against the closed form of axis boxes,
the stream contract of the `_dev` entry and the size errors."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import pair_dist_host as ph  # noqa: E402
import support_host as sh  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def L(tmp_path_factory):
    return ph.build(tmp_path_factory.mktemp("pair_dist_host"))


@pytest.fixture(scope="module")
def pa():
    import polytope_amd
    polytope_amd.solvers.default_solver = "hip"
    return polytope_amd


def same(dev, host, where=None):
    for k in ph.KEYS:
        a = dev[k].cpu().numpy() if hasattr(dev[k], "cpu") else dev[k]
        h = host[k]
        assert a.shape == h.shape, k
        if where is not None:
            a, h = a[where], h[where]
        view = np.int64 if a.dtype.itemsize == 8 else np.int32
        assert np.array_equal(np.ascontiguousarray(a).view(view), np.ascontiguousarray(h).view(view)), k


def on_device(pa, A, b, pairs, m, xc, **kw):
    """distance_pairs on CUDA tensors (the device-pointer entry) -> numpy."""
    import torch
    dev = torch.device("cuda", 0)
    t = lambda v: None if v is None else torch.as_tensor(np.ascontiguousarray(v)).to(dev)   # noqa: E731
    out = pa.batch.distance_pairs(t(A), t(b), t(pairs), m=t(m), xc=t(xc), **kw)
    return {k: None if v is None else v.cpu().numpy() for k, v in out.items()}


def centres(pa, A, b, m):
    """Chebyshev centres by the device (NaN where there is no usable one), given to the host build and the kernel alike."""
    ball = pa.cheby_ball_batch(A, b, m)
    ok = (ball["status"] == 0) & (ball["r"] > 0) & np.isfinite(ball["r"])
    return np.where(ok[:, None], ball["xc"], np.nan)


def cells(m_max, d, n, seed):
    """Ragged random cells, rows scaled, each translated by 0 .. 4 extents (a cell of few rows is unbounded: no centre)."""
    rng = np.random.default_rng(seed)
    A, b, m = sh.family("ragged", B=n, rng=rng, shape=(m_max, d))
    s = np.exp(rng.uniform(-1, 1, (n, m_max)))
    A *= s[:, :, None]
    b *= s
    m[0] = m_max
    m[1::2] = np.maximum(m[1::2], min(m_max, 2 * d))   # (half of the cells hold the box rows: bounded)
    return A, ph.translated(A, b, rng), m


@pytest.mark.parametrize("m_max", [16, 17, 33, 64])
@pytest.mark.parametrize("d", [1, 2, 3, 4])
def test_raw_answers_equal_the_host_build(L, pa, d, m_max):
    """Every RV x D instance, n = 40 ragged cells, K in 1, 2, 31, 33, 70: a tail tile at every RV (32 / 16 / 8 pairs per
    workgroup), lists that cross a tile boundary; on the device-pointer form one bad pair per list, which gets 255."""
    n = 40
    A, b, m = cells(m_max, d, n, 100 * d + m_max)
    xc = centres(pa, A, b, m)
    rng = np.random.default_rng(d + m_max)
    per = L.pair_dist_pairs_per_group(m_max)
    assert per in (32, 16, 8) and all(K % per for K in (1, 2, 31, 33, 70))
    settled = 0
    for K in (1, 2, 31, 33, 70):
        P = ph.pair_list(rng, n, max(K, 8))[:K]
        host = ph.run(L, A, b, xc, P, m)
        settled += int((host["status"] == 0).sum())
        same(pa.batch.distance_pairs(A, b, P, m=m, xc=xc, resolve=False), host)          # (host pointers)
        Pb = P.copy()
        Pb[K // 2] = [(3, 3), (n, 0), (0, -1)][K % 3]
        good = np.arange(K) != K // 2
        dev = on_device(pa, A, b, Pb, m, xc, resolve=False)
        same(dev, host, good)
        assert dev["status"][K // 2] == ph.PAIR_BAD
        assert all(np.all(np.isnan(dev[k][K // 2])) for k in ("dist", "lb", "x", "y"))
        bare = on_device(pa, A, b, P, m, xc, points=False, resolve=False)
        assert bare["x"] is None and bare["y"] is None
        assert ph.hb.same_bits(bare["dist"], host["dist"]) and np.array_equal(bare["status"], host["status"])
    assert settled > 30


@pytest.mark.parametrize("fam", ph.FAMILIES)
def test_soak_families_equal_the_host_build(L, pa, fam):
    """Every soak family at SOAK_SHAPES, 30 cells, 200 listed pairs."""
    rng = np.random.default_rng(sh.FAMILY_SEED[fam] + 700)
    for (m_max, d) in ph.SOAK_SHAPES:
        A, b, m = ph.cell_table(fam, m_max, d, 30, rng)
        xc = centres(pa, A, b, m)
        P = ph.pair_list(rng, 30)
        same(on_device(pa, A, b, P, m, xc, resolve=False), ph.run(L, A, b, xc, P, m))


def test_dev_entry_without_row_counts(L, pa):
    """m = None on CUDA tensors: the device-pointer entry with a NULL m (every cell has m_max rows); (17, 2): 32 row slots."""
    A, b, _ = cells(17, 2, 12, 171)
    xc = centres(pa, A, b, None)
    P = ph.pair_list(np.random.default_rng(172), 12, 40)
    same(on_device(pa, A, b, P, None, xc, resolve=False), ph.run(L, A, b, xc, P, None))


def test_dev_entry_on_a_second_stream(L, pa):
    """Tensors in, tensors out on torch's current stream: the call on a non-default stream while another kernel is in
    flight on a second one gives the host build's bits (the pattern of tests/test_nearest_gpu.py)."""
    import torch
    dev = torch.device("cuda", 0)
    A, b, m = cells(33, 4, 37, 5)
    xc = centres(pa, A, b, m)
    P = ph.pair_list(np.random.default_rng(6), 37, 300)
    host = ph.run(L, A, b, xc, P, m)
    s1, s2 = torch.cuda.Stream(dev), torch.cuda.Stream(dev)
    busy = torch.randn(2048, 2048, device=dev)
    torch.cuda.synchronize()
    with torch.cuda.stream(s2):
        for _ in range(20):
            busy = busy @ busy * 1e-3
    with torch.cuda.stream(s1):
        At, bt, mt, xt, Pt = (torch.as_tensor(v).to(dev, non_blocking=False) for v in (A, b, m, xc, P))
        out = pa.batch.distance_pairs(At, bt, Pt, m=mt, xc=xt, resolve=False)
        got = {k: v.clone() for k, v in out.items()}
    s1.synchronize()
    same(got, host)
    torch.cuda.synchronize()
    # resolve=True on tensors, the centres by cheby_ball_batch: tensors back, no status 1
    res = pa.batch.distance_pairs(At, bt, Pt, m=mt)
    assert res["dist"].is_cuda and not bool((res["status"] == 1).any())


@pytest.mark.parametrize("fam", ["random", "ragged", "dup", "flat"])
def test_resolved_answers_pass_the_duality_proof(pa, oracle, fam):
    """resolve=True (centres by cheby_ball_batch) on the CPU test's tables at (16, 1), (17, 2), (16, 3): no status 1 is left,
    every status 0 passes check (b), 2 only where the oracle finds a cell empty."""
    for T in ph.tables(oracle, fam)[:3]:
        for dev in (False, True):
            if dev:
                out = on_device(pa, T["A"], T["b"], T["pairs"], T["m"], None)
            else:
                out = pa.batch.distance_pairs(T["A"], T["b"], T["pairs"], m=T["m"])
            ph.check_statuses(T, out, resolved=True)
            ph.check_duality(oracle, T, out)
            # 2 only where the oracle's ball LP is infeasible or its radius is nothing at the LP tolerance (1e-9: a slab of
            # width zero is empty or not by rounding alone)
            i, j = T["pairs"][:, 0], T["pairs"][:, 1]
            empty = (T["r"] == -np.inf) | (T["r"] <= ph.TOL)
            assert not np.any((out["status"] == 2) & ~(empty[i] | empty[j]))
            assert (out["status"] == 0).sum() > 0.3 * out["status"].size


def test_polytope_and_region_calls(pa):
    """polytope.distance_pairs and set_distance on the 64-cell d = 2 box grid (cells one apart) against the closed form."""
    cells_ = [pa.box2poly([[2.0 * i, 2.0 * i + 1.0], [2.0 * j, 2.0 * j + 1.0]]) for i in range(8) for j in range(8)]
    lo = np.array([[2.0 * i, 2.0 * j] for i in range(8) for j in range(8)])
    hi = lo + 1.0
    rng = np.random.default_rng(12)
    P = ph.pair_list(rng, 64, 300)
    dist, x, y = pa.distance_pairs(cells_, P)
    ref = ph.box_distance(lo, hi, P)
    assert np.allclose(dist, ref, rtol=0, atol=1e-9 * 16) and np.allclose(np.linalg.norm(x - y, axis=1), dist, rtol=0, atol=1e-12)
    assert np.all(x >= lo[P[:, 0]] - 1e-8) and np.all(x <= hi[P[:, 0]] + 1e-8)
    assert np.all(y >= lo[P[:, 1]] - 1e-8) and np.all(y <= hi[P[:, 1]] + 1e-8)
    # an empty cell: inf and NaN points
    de, xe, _ = pa.distance_pairs([cells_[0], pa.Polytope()], [(0, 1)])
    assert de[0] == np.inf and np.all(np.isnan(xe[0]))
    # Polytope x Region: the minimum over the members, the lowest pair index on ties
    probe = pa.box2poly([[4.25, 4.75], [-3.0, -2.0]])     # below the cells (2, 0): nearest member 2 * 8 + 0 = 16, 2 away
    reg = pa.Region(cells_)
    dd, xx, yy, (ma, mb) = pa.set_distance(probe, reg)
    assert abs(dd - 2.0) <= 1e-9 and (ma, mb) == (0, 16) and abs(xx[1] + 2.0) <= 1e-9 and abs(yy[1]) <= 1e-9
    dr, xr, yr, (mr, mp) = pa.set_distance(reg, probe)
    assert abs(dr - 2.0) <= 1e-9 and (mr, mp) == (16, 0)
    tie = pa.box2poly([[1.25, 1.75], [0.0, 1.0]])          # between the cells (0, 0) and (1, 0), 0.25 from each
    assert pa.set_distance(tie, reg)[3] == (0, 0)
    assert pa.set_distance(cells_[0], cells_[9])[0] == pytest.approx(np.sqrt(2.0), abs=1e-9)
    pa.solvers.default_solver = "scipy"
    try:
        with pytest.raises(ValueError):
            pa.distance_pairs(cells_, P)
        with pytest.raises(ValueError):
            pa.set_distance(probe, reg)
    finally:
        pa.solvers.default_solver = "hip"


def test_size_errors(pa):
    """d = 5 and m_max = 65: PLP_EUNSUPPORTED from the C ABI (UnsupportedSize from Python); K = 0 and n = 0: OK, nothing runs;
    a bad pair in the host-pointer form: PLP_EINVAL (ValueError from Python)."""
    from polytope_amd import _lib
    lib, ctx = _lib.load(), _lib.context()
    buf = np.zeros(65 * 5 * 4)
    pr = np.array([[0, 1]], np.int32)
    st = np.full(4, 77, np.int32)
    p = lambda a: C.c_void_p(a.ctypes.data)   # noqa: E731

    mz = np.zeros(2, np.int32)

    def call(n, m_max, d, K, pairs=pr):
        return lib.plp_pair_dist(ctx.handle, n, m_max, d, p(buf), p(buf), p(mz), p(buf), K, p(pairs), p(buf), None, None, None, p(st))
    assert call(2, 6, 5, 1) == _lib.PLP_EUNSUPPORTED and call(2, 65, 3, 1) == _lib.PLP_EUNSUPPORTED
    assert call(2, 6, 3, 0) == _lib.PLP_OK and call(0, 6, 3, 1) == _lib.PLP_OK and np.all(st == 77)
    assert call(2, 6, 3, 1, np.array([[1, 1]], np.int32)) == _lib.PLP_EINVAL
    assert call(2, 6, 3, 1, np.array([[0, 2]], np.int32)) == _lib.PLP_EINVAL and np.all(st == 77)
    assert call(2, 6, 3, 1) == _lib.PLP_OK and st[0] == 3    # (two cells without rows: unbounded)
    with pytest.raises(_lib.UnsupportedSize):
        pa.batch.distance_pairs(np.zeros((2, 6, 5)), np.ones((2, 6)), pr)
    with pytest.raises(_lib.UnsupportedSize):
        pa.batch.distance_pairs(np.zeros((2, 65, 3)), np.ones((2, 65)), pr)
    with pytest.raises(ValueError):
        pa.batch.distance_pairs(np.zeros((2, 6, 3)), np.ones((2, 6)), np.array([[1, 1]], np.int32))
    out = pa.batch.distance_pairs(np.zeros((2, 6, 3)), np.ones((2, 6)), np.zeros((0, 2), np.int32))
    assert out["dist"].shape == (0,) and out["x"].shape == (0, 3)
