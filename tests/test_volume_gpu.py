"""GPU: the device volume (csrc/plp_volume.hip through polytope_amd.batch.volume_batch and polytope.volume) against the
reference's hit counts and floats (g28), against the host build of the same arithmetic (tests/cabi/volume_host.cpp) bit
for bit in the counts, and against the sample-upload path it replaces (polytope._volume_by_samples)."""
import itertools
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import polytope_amd as pa  # noqa: E402
from polytope_amd import batch, solvers  # noqa: E402
from polytope_amd import polytope as alg  # noqa: E402
import volume_host as vh  # noqa: E402
from conftest import load_golden  # noqa: E402
from test_volume_host import g28_cases  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture
def hip_backend():
    saved = solvers.default_solver
    solvers.default_solver = "hip"
    yield
    solvers.default_solver = saved


@pytest.fixture(scope="module")
def L(tmp_path_factory):
    return vh.build(tmp_path_factory.mktemp("volume_host"))


def pack(cases):
    B, d = len(cases), cases[0]["d"]
    m_max = max(c["m"] for c in cases)
    A = np.zeros((B, m_max, d))
    b = np.zeros((B, m_max))
    for k, c in enumerate(cases):
        A[k, :c["m"]], b[k, :c["m"]] = c["A"], c["b"]
    return A, b, np.array([c["m"] for c in cases], np.int32)


def g28_groups():
    groups = {}
    for c in g28_cases():
        groups.setdefault((c["d"], c["N"]), []).append(c)
    return groups


# ------------------------------------------------------------------------------------------ 4: g28
def test_g28_reference_boxes_batched_and_single():
    """The reference's boxes passed in: its hit counts and its float, in one batch per (d, N) and one by one; numpy in
    and torch CUDA tensors in."""
    import torch
    n = 0
    for (d, N), cases in g28_groups().items():
        A, b, m = pack(cases)
        lb = np.array([c["lb"] for c in cases])
        ub = np.array([c["ub"] for c in cases])
        seeds = [c["seed"] for c in cases]
        res = batch.volume_batch(A, b, m=m, nsamples=N, seed=seeds, lb=lb, ub=ub)
        assert res["nsamples"] == N and not res["flags"].any()
        assert [int(h) for h in res["hits"]] == [c["hits"] for c in cases], (d, N)
        assert [float(v) for v in res["volume"]] == [c["vol"] for c in cases], (d, N)
        dev = torch.device("cuda:0")
        rt = batch.volume_batch(torch.as_tensor(A).to(dev), torch.as_tensor(b).to(dev), m=torch.as_tensor(m).to(dev),
                                nsamples=N, seed=seeds, lb=torch.as_tensor(lb).to(dev), ub=torch.as_tensor(ub).to(dev))
        assert np.array_equal(rt["hits"].cpu().numpy(), res["hits"].astype(np.int32))
        assert np.array_equal(rt["volume"].numpy(), res["volume"])
        for c in cases:
            r1 = batch.volume_batch(c["A"][None], c["b"][None], nsamples=N, seed=c["seed"], lb=c["lb"][None],
                                    ub=c["ub"][None])
            assert int(r1["hits"][0]) == c["hits"] and float(r1["volume"][0]) == c["vol"], c["k"]
            n += 1
    assert n >= 200


def test_g28_own_boxes():
    """The library's own bbox_batch boxes (no lb / ub given): the same hit counts -- every sample of g28 is at least
    1e-9 from every row -- and the volume to rel 1e-9."""
    for (d, N), cases in g28_groups().items():
        A, b, m = pack(cases)
        res = batch.volume_batch(A, b, m=m, nsamples=N, seed=[c["seed"] for c in cases])
        assert not res["flags"].any()
        assert np.allclose(res["lb"], [c["lb"] for c in cases], atol=1e-9, rtol=1e-12)
        assert [int(h) for h in res["hits"]] == [c["hits"] for c in cases], (d, N)
        for v, c in zip(res["volume"], cases):
            assert float(v) == pytest.approx(c["vol"], rel=1e-9), c["k"]


def test_g28_through_volume(hip_backend):
    """polytope.volume on 'hip' with the default and the explicit sample counts: hits equal, value to rel 1e-9 (own box)."""
    for c in g28_cases():
        P = alg.Polytope(c["A"], c["b"], normalize=False)
        v = alg.volume(P, nsamples=None if c["ns"] < 0 else c["ns"], seed=c["seed"])
        l, u = P.bounding_box
        assert int(round(v / np.prod(u - l) * c["N"])) == c["hits"], c["k"]
        assert v == pytest.approx(c["vol"], rel=1e-9) and P.volume == v


# ------------------------------------------------------------------------------------------ 5: device against host build
def mixed_batch(rng, B, d, m_max):
    """B ragged polytopes around the origin: a box of half-width 1 plus random cuts, rows zero-padded to m_max."""
    A = np.zeros((B, m_max, d))
    b = np.zeros((B, m_max))
    m = np.zeros(B, np.int32)
    for k in range(B):
        extra = int(rng.integers(0, m_max - 2 * d + 1)) if m_max > 2 * d else 0
        C = rng.standard_normal((extra, d))
        C /= np.linalg.norm(C, axis=1, keepdims=True) if extra else 1.0
        rows = np.vstack([C, np.eye(d), -np.eye(d)])
        rhs = np.hstack([rng.uniform(0.3, 1.2, extra) * np.sqrt(d), np.ones(2 * d)])
        perm = rng.permutation(len(rhs))
        m[k] = len(rhs)
        A[k, :m[k]], b[k, :m[k]] = rows[perm], rhs[perm]
    lb = -np.ones((B, d)) - rng.random((B, d)) * 0.1
    ub = np.ones((B, d)) + rng.random((B, d)) * 0.1
    return A, b, m, lb, ub


def test_device_equals_host_build(L):
    """~10 000 mixed polytopes, d = 1..16, ragged m, N from 1 to 50 000: batches large enough for one tile per polytope
    and small enough for many, N that fills the last pass and N that does not; then B = 1 with N = 10^7.  hits bit for bit."""
    rng = np.random.default_rng(55)
    total = 0
    for d in range(1, 17):
        chunk = 256 * (4 if d <= 8 else 2)
        plan = [(420, int(rng.integers(1, 600))), (120, 3000), (40, chunk), (24, chunk + 1), (12, 3 * chunk - 1),
                (8, 50000), (3, 4 * chunk), (2, int(rng.integers(20000, 50000))), (1, 1), (1, 63), (1, 64), (1, 65)]
        for B, N in plan:
            m_max = int(rng.integers(2 * d, 65)) if 2 * d < 64 else 64
            A, b, m, lb, ub = mixed_batch(rng, B, d, max(m_max, 2 * d))
            seeds = [int(s) for s in rng.integers(0, 2 ** 62, B)]
            st, inc = batch._pcg64_words(seeds)
            want, wfl = vh.hits(L, A, b, lb, ub, st, inc, N, m=m)
            res = batch.volume_batch(A, b, m=m, nsamples=N, seed=seeds, lb=lb, ub=ub)
            assert np.array_equal(res["flags"], wfl) and not wfl.any()
            assert np.array_equal(res["hits"], want), (d, B, N, np.nonzero(res["hits"] != want)[0][:5])
            total += B
    assert total >= 10000
    for d, m_max in ((3, 16), (12, 30)):
        A, b, m, lb, ub = mixed_batch(rng, 1, d, m_max)
        N = 10 ** 7 if d == 3 else 10 ** 6 + 7
        st, inc = batch._pcg64_words([77])
        want, _ = vh.hits(L, A, b, lb, ub, st, inc, N, m=m)
        res = batch.volume_batch(A, b, m=m, nsamples=N, seed=77, lb=lb, ub=ub)
        assert int(res["hits"][0]) == int(want[0]) and 0 < int(want[0]) < N


def test_grid_stride_loop(L, monkeypatch):
    """More work items than workgroups (the launcher caps the grid at 2^22, which no test batch reaches: PLP_VOLUME_MAX_GRID
    lowers the cap): a workgroup takes several (polytope, tile) items in turn, counts as the host build's."""
    rng = np.random.default_rng(22)
    for d, B, N, cap in ((3, 700, 2500, 64), (2, 5, 40000, 7), (12, 90, 1500, 1)):
        A, b, m, lb, ub = mixed_batch(rng, B, d, 30)
        seeds = [int(s) for s in rng.integers(0, 2 ** 62, B)]
        st, inc = batch._pcg64_words(seeds)
        want, _ = vh.hits(L, A, b, lb, ub, st, inc, N, m=m)
        monkeypatch.setenv("PLP_VOLUME_MAX_GRID", str(cap))
        res = batch.volume_batch(A, b, m=m, nsamples=N, seed=seeds, lb=lb, ub=ub)
        monkeypatch.delenv("PLP_VOLUME_MAX_GRID")
        assert np.array_equal(res["hits"], want), (d, B, N, cap)


def test_flags_and_limits():
    """Box not finite / no rows: flagged, hits 0, volume nan; beyond d <= 16, m <= 64 and N <= 2^31 - 1 the library says so."""
    A = np.zeros((3, 4, 2))
    b = np.ones((3, 4))
    A[:] = np.array([[1, 0], [-1, 0], [0, 1], [0, -1.0]])
    lb = np.array([[-1, -1], [-np.inf, -1], [-1, -1.0]])
    ub = np.ones((3, 2))
    res = batch.volume_batch(A, b, m=np.array([4, 4, 0], np.int32), nsamples=100, seed=1, lb=lb, ub=ub)
    assert list(res["flags"]) == [0, batch.VF_NONFINITE, batch.VF_NOROWS]
    assert list(res["hits"]) == [100, 0, 0] and res["volume"][0] == 4.0 and np.isnan(res["volume"][1:]).all()
    from polytope_amd import _lib
    with pytest.raises(_lib.UnsupportedSize):
        batch.volume_batch(np.zeros((1, 65, 2)), np.ones((1, 65)), seed=1, lb=-np.ones((1, 2)), ub=np.ones((1, 2)))
    with pytest.raises(_lib.UnsupportedSize):
        batch.volume_batch(np.zeros((1, 4, 17)), np.ones((1, 4)), seed=1, lb=-np.ones((1, 17)), ub=np.ones((1, 17)))


# ------------------------------------------------------------------------------------------ 6: against the parent's path
def random_polytope(rng, d):
    m = int(rng.integers(d + 1, 40))
    A = rng.standard_normal((m, d))
    A /= np.linalg.norm(A, axis=1, keepdims=True)
    return alg.Polytope(np.vstack([A, np.eye(d), -np.eye(d)]), np.hstack([rng.uniform(0.5, 1.5, m), np.full(2 * d, 2.0)]))


def test_volume_equals_sample_upload_path(hip_backend):
    """volume(P, ns, seed) == _volume_by_samples(P, ns, seed) as floats (same box, same samples, same arithmetic)."""
    rng = np.random.default_rng(6)
    for t in range(300):
        d = int(rng.integers(1, 9)) if t % 10 else int(rng.choice([12, 16]))
        P = random_polytope(rng, d)
        ns = None if t % 3 == 0 else int(rng.choice([1, 63, 64, 65, 257, 1000, 3000, 20000]))
        seed = int(rng.integers(0, 2 ** 62))
        new = alg.volume(P, ns, seed)
        assert P._volume == new
        old = alg._volume_by_samples(P, ns, seed)
        assert new == old, (t, d, ns, seed, new, old)


def _grid_cells(shape):
    d = len(shape)
    return [alg.box2poly([[idx[k] / shape[k], (idx[k] + 1) / shape[k]] for k in range(d)])
            for idx in itertools.product(*[range(n) for n in shape])]


def test_region_1000_cells_equals_the_loop(hip_backend, monkeypatch):
    """volume(Region) of a 10 x 10 x 10 x 1 ... d = 4 grid of 1000 boxes: ONE volume_batch call; with the seeds that call
    drew fed back one by one to the sample-upload path, every member's _volume and the sum in member order are equal."""
    cells = _grid_cells((10, 10, 5, 2))
    assert len(cells) == 1000
    R = alg.Region(cells)
    calls = []
    real = batch.volume_batch

    def spy(*a, **kw):
        res = real(*a, **kw)
        calls.append(res)
        return res
    monkeypatch.setattr(batch, "volume_batch", spy)
    tot = alg.volume(R)
    assert len(calls) == 1 and len(calls[0]["seeds"]) == 1000 and calls[0]["nsamples"] == 10000
    assert R._volume == tot
    want = 0.0
    for p, sd in zip(R.list_poly, calls[0]["seeds"]):
        q = p.copy()
        q.bbox = p.bbox
        v = alg._volume_by_samples(q, None, sd)
        assert p._volume == v
        want += v
    assert tot == want
    assert tot == pytest.approx(1.0, rel=1e-6)


# ------------------------------------------------------------------------------------------ 7: contract
def test_object_flows_and_edge_members(hip_backend, monkeypatch):
    """is_subset / == / <= on the g13 objects, Partition.refines and is_cover on the g16 objects give the fixtures' verdicts
    through the new path (volume_batch is what ran);
    unbounded, empty, flat and over-the-limit members: the parent's values."""
    g = load_golden("g13_volume_subset.npz")
    ncalls = [0]
    real = batch.volume_batch

    def spy(*a, **kw):
        ncalls[0] += 1
        return real(*a, **kw)
    monkeypatch.setattr(batch, "volume_batch", spy)

    def build(tag, key):
        ps = [(int(g[f"{tag}_{key}_m"][k]), g[f"{tag}_{key}_Ab"][k]) for k in range(int(g[f"{tag}_{key}_n"]))]
        mmax = max(m for m, _ in ps)
        d = g[f"{tag}_{key}_Ab"].shape[1] // mmax - 1
        polys = [alg.Polytope(row[:m * (d + 1)].reshape(m, d + 1)[:, :d], row[:m * (d + 1)].reshape(m, d + 1)[:, d],
                              normalize=False) for m, row in ps]
        return alg.Region(polys) if int(g[f"{tag}_{key}_isreg"]) else polys[0]

    for tag in g["rel_names"]:
        tag = str(tag)
        X, Y = build(tag, "X"), build(tag, "Y")
        got = [bool(alg.is_subset(X.copy(), Y.copy())), bool(alg.is_subset(Y.copy(), X.copy())),
               bool(X.copy() == Y.copy()), bool(X.copy() <= Y.copy()), bool(X.copy() >= Y.copy()),
               bool(X.copy() != Y.copy())]
        assert got == [bool(v) for v in g[tag + "_res"]], tag
    assert ncalls[0] > 0
    # g16: Partition.refines on every recorded pair and is_cover of every partition, verdicts as the fixture holds them
    import warnings
    from test_dropin_root import _partition
    g16 = load_golden("g16_partition.npz")
    n1 = ncalls[0]
    for pair, want in zip(g16["refines_pairs"], g16["refines"]):
        a, c = str(pair).split(">")
        assert _partition(pa, g16, a, "Partition").refines(_partition(pa, g16, c, "Partition")) == bool(want), pair
    assert len(g16["refines_pairs"]) > 0 and ncalls[0] > n1   # (the pairs no bounding-box argument settles sample volumes)
    names = sorted({nm for pair in g16["refines_pairs"] for nm in str(pair).split(">")})
    for name in names:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            assert _partition(pa, g16, name).is_cover() == bool(g16[name + "_cover"]), name
    box = alg.box2poly([[0, 1], [0, 1]])
    half = alg.Polytope(np.array([[1.0, 0], [-1, 0], [0, 1], [0, -1]]), np.array([1.0, 0, 1, 1]))   # [0, 1] x [-1, 1]
    unb = alg.Polytope(np.array([[1.0, 0], [0, 1], [0, -1]]), np.array([1.0, 1, 0]))               # x unbounded below
    flat = alg.Polytope(np.array([[1.0, 0], [-1, 0], [0, 1], [0, -1]]), np.array([1.0, -1, 1, 0]))  # x = 1
    rng = np.random.default_rng(3)
    Ab = rng.standard_normal((70, 2))
    Ab /= np.linalg.norm(Ab, axis=1, keepdims=True)
    big = alg.Polytope(np.vstack([Ab, np.eye(2), -np.eye(2)]), np.hstack([np.full(70, 1.0), np.full(4, 2.0)]))
    assert big.A.shape[0] > 64
    n0 = ncalls[0]
    assert alg.volume(big, seed=3) == alg._volume_by_samples(big, None, 3)     # over the limits: the upload path
    vu, vo = alg.volume(unb, seed=3), alg._volume_by_samples(unb, None, 3)     # box not finite: the upload path
    assert (np.isnan(vu) and np.isnan(vo)) or vu == vo
    assert ncalls[0] == n0
    assert alg.volume(flat) == 0.0 and flat._volume is None
    assert alg.volume(alg.Polytope()) == 0.0
    R = alg.Region([box.copy(), flat.copy(), half.copy()])
    tot = alg.volume(R)
    assert R.list_poly[1]._volume is None                                       # the gate: untouched, contributes 0.0
    assert tot == R.list_poly[0]._volume + 0.0 + R.list_poly[2]._volume
    assert R.list_poly[0]._volume == 1.0 and R.list_poly[2]._volume == pytest.approx(2.0, rel=0.1)
    with pytest.raises(ValueError, match="`nsamples` must be >= 1"):
        alg.volume(box.copy(), nsamples=0)
    with pytest.raises(ValueError, match="noninteger"):
        alg.volume(box.copy(), nsamples=2.5)


# ------------------------------------------------------------------------------------------ 8: no sample traffic
def test_uploads_only_the_generator_state():
    import torch
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(8)
    B, d = 500, 3
    A, b, m, lb, ub = mixed_batch(rng, B, d, 16)
    At, bt, mt, lt, ut = (torch.as_tensor(v).to(dev) for v in (A, b, m, lb, ub))
    for N in (100, 3000, 200000):
        before = batch.h2d_bytes
        res = batch.volume_batch(At, bt, m=mt, nsamples=N, seed=list(range(B)), lb=lt, ub=ut)
        assert batch.h2d_bytes - before == B * 32, N
        assert res["hits"].is_cuda and int(res["hits"].sum()) > 0
    before = batch.h2d_bytes
    res = batch.volume_batch(At, bt, m=mt, seed=5)    # boxes from bbox_batch, handed on as device arrays
    assert batch.h2d_bytes - before == B * 32 and res["lb"].is_cuda and res["nsamples"] == 3000
