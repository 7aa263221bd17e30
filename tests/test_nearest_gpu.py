"""GPU: nearest_kernel<D, RV> (polytope_amd/csrc/plp_nearest.hip) behind batch.nearest_batch.

Raw device answers (resolve=False) equal the host build of the same source (tests/cabi/nearest_host.cpp) BIT FOR BIT --
dist, x, face, lam, status -- at every (D, RV) instance, with tail tiles, across the K-chunk boundary (the second grid
index), shared and per-polytope points and on every soak family.  Resolved answers are held to the references of
tests/nearest_host.py with the tolerances of tests/test_nearest_host.py (1e-9 E), and no status 1 is left.  Then the
object-level calls, the stream contract of the `_dev` entry and the size errors."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import nearest_host as nh  # noqa: E402
import support_host as sh  # noqa: E402

pytestmark = pytest.mark.gpu
KEYS = ("dist", "x", "face", "lam", "status")


@pytest.fixture(scope="module")
def L(tmp_path_factory):
    return nh.build(tmp_path_factory.mktemp("nearest_host"))


@pytest.fixture(scope="module")
def pa():
    import polytope_amd
    polytope_amd.solvers.default_solver = "hip"
    return polytope_amd


def same(dev, host):
    for k in KEYS:
        if host[k] is None:
            assert dev[k] is None
            continue
        a = dev[k].cpu().numpy() if hasattr(dev[k], "cpu") else dev[k]
        assert a.shape == host[k].shape, k
        assert np.array_equal(np.ascontiguousarray(a).view(np.int64 if a.dtype.itemsize == 8 else np.int32),
                              np.ascontiguousarray(host[k]).view(np.int64 if a.dtype.itemsize == 8 else np.int32)), k


def on_device(pa, A, b, X, m, **kw):
    """nearest_batch on CUDA tensors (the device-pointer entry: a NaN point is an input like any other there; the
    host-pointer entry refuses it when the context checks for finite input) -> numpy."""
    import torch
    dev = torch.device("cuda", 0)
    out = pa.nearest_batch(*(torch.as_tensor(np.ascontiguousarray(v)).to(dev) for v in (A, b, X)), m=torch.as_tensor(m).to(dev), **kw)
    return {k: None if v is None else (v.cpu().numpy().view(np.uint64) if k == "face" else v.cpu().numpy()) for k, v in out.items()}


def polytopes(m_max, d, B, seed):
    """Ragged random polytopes around the origin (box rows first where they fit), some rows scaled, one member empty."""
    rng = np.random.default_rng(seed)
    A, b, m = sh.family("ragged", B=B, rng=rng, shape=(m_max, d))
    A *= np.exp(rng.uniform(-1, 1, (B, m_max, 1)))
    m[0] = m_max
    if B > 3 and m_max >= 2:
        A[3, 0], A[3, 1] = 1.0, -1.0
        A[3, :2, 1:] = 0.0
        b[3, 0], b[3, 1] = 1.0, -2.0    # x_0 <= 1 and x_0 >= 2
        m[3] = max(m[3], 2)
    return A, b, m


@pytest.mark.parametrize("m_max", [16, 17, 33, 64])
@pytest.mark.parametrize("d", [1, 2, 3, 4])
def test_raw_answers_equal_the_host_build(L, pa, d, m_max):
    """Every RV x D instance, B = 40 (a tail tile wherever 40 is no multiple of the polytopes per workgroup), K in 1, 9, 33,
    70, shared and per-polytope points (some NaN, some inside, some far)."""
    A, b, m = polytopes(m_max, d, 40, 100 * d + m_max)
    rng = np.random.default_rng(d + m_max)
    for K in (1, 9, 33, 70):
        for shared in (True, False):
            X = 2.5 * rng.standard_normal((K, d) if shared else (40, K, d))
            X.reshape(-1, d)[::7] *= 0.1
            X.reshape(-1, d)[5::11] *= 300.0
            if K > 1:
                X.reshape(-1, d)[1, 0] = np.nan
            host = nh.run(L, A, b, X, m)
            assert (host["status"] == 0).sum() > 0.5 * host["status"].size
            same(on_device(pa, A, b, X, m, faces=True, resolve=False), host)
    assert 40 % L.nearest_polytopes_per_group(1, m_max) != 0   # (K = 1: a tail tile)


def test_second_grid_index(L, pa):
    """K just above the K-chunk length (8 rounds of 64 lanes = 512 points; K >= 33 means one polytope per workgroup), and
    just above two chunks: the second grid index, with a ragged last chunk."""
    for (m_max, d, B, K) in ((16, 3, 3, 513), (33, 4, 2, 1030)):
        chunk = L.nearest_chunk_points(K, m_max)
        assert chunk < K < 3 * chunk + 8
        A, b, m = polytopes(m_max, d, B, K)
        rng = np.random.default_rng(K)
        for shared in (True, False):
            X = 2.5 * rng.standard_normal((K, d) if shared else (B, K, d))
            same(pa.nearest_batch(A, b, X, m=m, faces=True, resolve=False), nh.run(L, A, b, X, m))   # (host pointers)


def test_dev_entry_without_row_counts(L, pa):
    """m = None on CUDA tensors: the device-pointer entry with a NULL m (every polytope has m_max rows), which the other
    tests reach through host pointers only; (17, 2): 32 row slots, B = 5 and K = 3 a tail tile."""
    import torch
    dev = torch.device("cuda", 0)
    A, b, _ = polytopes(17, 2, 5, 171)
    X = 2.5 * np.random.default_rng(172).standard_normal((5, 3, 2))
    out = pa.nearest_batch(*(torch.as_tensor(v).to(dev) for v in (A, b, X)), faces=True, resolve=False)
    same(out, nh.run(L, A, b, X, None))


@pytest.mark.parametrize("fam", nh.FAMILIES)
def test_soak_families_equal_the_host_build(L, pa, fam):
    """Every soak family at SOAK_SHAPES, B = 30, K = 7 normal points + one NaN, shared and per polytope."""
    rng = np.random.default_rng(sh.FAMILY_SEED[fam] + 900)
    for (m_max, d) in nh.SOAK_SHAPES:
        A, b, m = sh.family(fam, B=30, rng=rng, shape=(m_max, d))
        Xo = 3.0 * rng.standard_normal((30, 8, d))
        Xo[:, 7] = np.nan
        for X in (Xo, Xo[0]):
            host = nh.run(L, A, b, X, m)
            same(on_device(pa, A, b, X, m, faces=True, resolve=False), host)
            bare = on_device(pa, A, b, X, m, points=False, resolve=False)
            assert bare["x"] is None and bare["face"] is None and bare["lam"] is None
            assert nh.hb.same_bits(bare["dist"], host["dist"]) and np.array_equal(bare["status"], host["status"])


@pytest.mark.parametrize("fam", ["random", "dup", "flat", "degenerate"])
def test_resolved_answers_equal_the_reference(pa, oracle, fam):
    """resolve=True against the numpy reference (the cases of the CPU test at (16, 1), (17, 2), (16, 3); for `degenerate` the
    empty set / single point / m = 0 / zero row by hand): no status 1 is left, NaN points get 4."""
    if fam == "degenerate":
        cases = [sh.memo(("nearest", "hand"), lambda: nh.hand_case(oracle))]
    else:
        cases = sh.memo(("nearest3", fam), lambda: nh.soak_cases(oracle, fam, sh.FAMILY_SEED[fam], shapes=nh.SOAK_SHAPES[:3], B=nh.B_SOAK))
    for case in cases:
        for layout in ("shared", "own"):
            out = on_device(pa, case["A"], case["b"], case[layout][0], case["m"], faces=True)
            nh.check_case(case, layout, out, separated=fam in nh.SEPARATED, resolved=True)
    if fam == "degenerate":
        hand = cases[-1]
        out = on_device(pa, hand["A"], hand["b"], hand["own"][0], hand["m"])
        fin = np.isfinite(hand["own"][0]).all(axis=2)
        assert np.all(out["status"][0][fin[0]] == 2) and np.all(out["status"][3][fin[3]] == 2)
        assert np.all(out["status"][1][fin[1]] == 0) and np.allclose(out["x"][1][fin[1]], [0.5, 0.25, 0.0], rtol=0, atol=1e-9)
        assert np.all(out["status"][2][fin[2]] == 0) and np.array_equal(out["x"][2][fin[2]], hand["own"][0][2][fin[2]])
        assert np.all(out["status"][~fin] == 4)


def test_dev_entry_on_a_second_stream(L, pa):
    """Tensors in, tensors out on torch's current stream: the call on a non-default stream while another kernel is in
    flight on a second one gives the host build's bits (the pattern of tests/test_streams_gpu.py)."""
    import torch
    dev = torch.device("cuda", 0)
    A, b, m = polytopes(33, 4, 37, 5)
    X = 2.5 * np.random.default_rng(6).standard_normal((37, 70, 4))
    host = nh.run(L, A, b, X, m)
    s1, s2 = torch.cuda.Stream(dev), torch.cuda.Stream(dev)
    busy = torch.randn(2048, 2048, device=dev)
    torch.cuda.synchronize()
    with torch.cuda.stream(s2):
        for _ in range(20):
            busy = busy @ busy * 1e-3
    with torch.cuda.stream(s1):
        At, bt, mt, Xt = (torch.as_tensor(v).to(dev, non_blocking=False) for v in (A, b, m, X))
        out = pa.nearest_batch(At, bt, Xt, m=mt, faces=True, resolve=False)
        got = {k: v.clone() for k, v in out.items()}
    s1.synchronize()
    same(got, host)
    torch.cuda.synchronize()
    # resolve=True on tensors: tensors back, no status 1
    res = pa.nearest_batch(At, bt, Xt, m=mt)
    assert res["dist"].is_cuda and not bool((res["status"] == 1).any())


def test_polytope_and_region_calls(pa):
    """polytope.nearest / distance on a Polytope and on a 64-cell d = 2 Region equal the per-member minimum of nearest_batch
    (lowest index on ties); Partition.nearest returns the containing region with distance 0 where locate finds one."""
    rng = np.random.default_rng(12)
    cells = [pa.box2poly([[i, i + 1.0], [j, j + 1.0]]) for i in range(8) for j in range(8)]
    reg = pa.Region(cells)
    pts = np.hstack([rng.uniform(-3, 11, (2, 200)), np.array([[4.0, 9.5, -1.0], [4.0, 3.0, 8.0]])])   # (4, 4): a 4-cell corner
    x, dist, member = pa.nearest(reg, pts)
    A = np.stack([c.A for c in cells])
    b = np.stack([c.b for c in cells])
    raw = pa.nearest_batch(A, b, np.ascontiguousarray(pts.T))
    assert np.all(raw["status"] == 0)
    arg = np.argmin(raw["dist"], axis=0)
    assert np.array_equal(member, arg.astype(np.int32)) and np.array_equal(dist, raw["dist"][arg, np.arange(pts.shape[1])])
    assert np.array_equal(x, raw["x"][arg, np.arange(pts.shape[1])])
    assert np.array_equal(reg.distance(pts), dist) and np.array_equal(pa.distance(reg, pts), dist)
    box = np.clip(pts, 0.0, 8.0)
    assert np.allclose(dist, np.linalg.norm(pts - box, axis=0), rtol=0, atol=1e-12) and np.allclose(x.T, box, rtol=0, atol=1e-12)
    xp, dp = cells[9].nearest(pts)
    assert np.array_equal(dp, raw["dist"][9]) and np.array_equal(xp, raw["x"][9]) and np.array_equal(cells[9].distance(pts), dp)
    part = pa.Partition(reg)
    part.regions = [pa.Region(cells[8 * i:8 * i + 8]) for i in range(8)]
    ridx, rd = part.nearest(pts)
    loc = part.locate(pts)
    assert (loc >= 0).sum() > 30 and (loc < 0).sum() > 30
    assert np.array_equal(ridx[loc >= 0], loc[loc >= 0]) and np.all(rd[loc >= 0] == 0.0)
    assert np.array_equal(ridx, (member // 8).astype(np.int32)) and np.array_equal(rd, dist)
    pa.solvers.default_solver = "scipy"
    try:
        with pytest.raises(ValueError):
            pa.nearest(reg, pts)
    finally:
        pa.solvers.default_solver = "hip"


def test_size_errors(pa):
    """d = 5, m_max = 65 and K = 0: PLP_EUNSUPPORTED from the C ABI (UnsupportedSize / ValueError from Python); B = 0: OK."""
    from polytope_amd import _lib
    lib, ctx = _lib.load(), _lib.context()
    buf = np.zeros(65 * 5 * 4)
    st = np.zeros(16, np.int32)
    p = lambda a: C.c_void_p(a.ctypes.data)   # noqa: E731

    def call(B, m_max, d, K):
        return lib.plp_nearest_batch(ctx.handle, B, m_max, d, p(buf), p(buf), None, K, p(buf), 1, p(buf), None, None, None, p(st))
    assert call(1, 6, 5, 1) == _lib.PLP_EUNSUPPORTED and call(1, 65, 3, 1) == _lib.PLP_EUNSUPPORTED
    assert call(1, 6, 3, 0) == _lib.PLP_EUNSUPPORTED and call(0, 6, 3, 1) == _lib.PLP_OK and call(1, 6, 3, 1) == _lib.PLP_OK
    with pytest.raises(_lib.UnsupportedSize):
        pa.nearest_batch(np.zeros((1, 6, 5)), np.ones((1, 6)), np.zeros((1, 5)))
    with pytest.raises(_lib.UnsupportedSize):
        pa.nearest_batch(np.zeros((1, 65, 3)), np.ones((1, 65)), np.zeros((1, 3)))
    with pytest.raises(ValueError):
        pa.nearest_batch(np.zeros((1, 6, 3)), np.ones((1, 6)), np.zeros((0, 3)))
    out = pa.nearest_batch(np.zeros((0, 6, 3)), np.ones((0, 6)), np.zeros((4, 3)))
    assert out["dist"].shape == (0, 4)
