"""GPU: projection() on 'hip' against the reference's answers (g27), and projection_batch (polytope_amd/batch.py: the
Fourier-Motzkin step kernels of csrc/plp_fm.hip between fused reduces) step by step against the host build of the same
row arithmetic (tests/cabi/fm_host.cpp) and the oracle's reduce, and end to end against per-polytope projection()."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import polytope_amd as pa  # noqa: E402
from polytope_amd import solvers  # noqa: E402
from polytope_amd import polytope as alg  # noqa: E402
import fm_host  # noqa: E402
from test_projection import g27_cases, run_case, check_case  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture
def hip_backend():
    saved = solvers.default_solver
    solvers.default_solver = "hip"
    yield
    solvers.default_solver = saved


@pytest.fixture(scope="module")
def fmlib(tmp_path_factory):
    return fm_host.build(tmp_path_factory.mktemp("fm"))


def test_g27_hip(hip_backend):
    for c in g27_cases():
        check_case(c, run_case(c))


def tulip_batch(rng, B, n, k, mt):
    """B TuLiP-shaped polytopes (state box, input box, mt target rows through x+ = Ax + Bu), rows as Polytope holds them."""
    d = n + k
    m = 2 * d + mt
    A = np.zeros((B, m, d))
    b = np.zeros((B, m))
    for t in range(B):
        Ad = np.eye(n) + 0.2 * rng.standard_normal((n, n))
        Bd = rng.standard_normal((n, k))
        rows = [np.eye(d)[i] for i in range(d)] + [-np.eye(d)[i] for i in range(d)]
        rhs = list(1.0 + rng.random(d)) + list(1.0 + rng.random(d))
        for _ in range(mt):
            a = rng.standard_normal(n)
            a /= np.linalg.norm(a)
            rows.append(np.hstack([a @ Ad, a @ Bd]))
            rhs.append(0.5 + rng.random())
        P = pa.Polytope(np.array(rows), np.array(rhs))
        A[t], b[t] = P.A, P.b
    return A, b


def sphere(rng, m, d):
    X = rng.standard_normal((m, d))
    X /= np.linalg.norm(X, axis=1)[:, None]
    return X, np.ones(m)


@pytest.mark.parametrize("family", ["tulip", "wide"])
def test_step_by_step_against_host_and_oracle(fmlib, oracle, family):
    rng = np.random.default_rng(11)
    if family == "tulip":
        A, b = tulip_batch(rng, 2000, 3, 2, 12)
    else:   # 31 facets of a sphere in R^5: the step forms ~200 rows (the LDS reduce); one step
        A = np.zeros((400, 31, 5))
        b = np.zeros((400, 31))
        for t in range(400):
            X, h = sphere(rng, 31, 5)
            P = pa.Polytope(X, h)
            A[t], b[t] = P.A, P.b
    B, m, d = A.shape
    res = pa.reduce_batch(A, b)
    ora = oracle.reduce_batch(A, b)
    assert np.array_equal(res["keep"], ora["keep"])
    keep, flags = res["keep"], res["flags"]
    A_cur, b_cur, m_cur = A, b, None
    first = True
    for col in ((4, 3) if family == "tulip" else (4,)):
        cnt = pa.batch.fm_count(A_cur, b_cur, col, m=m_cur, keep=keep, flags=flags, first=first)
        Ao, bo, mo = pa.batch.fm_emit(A_cur, b_cur, col, int(cnt.max()), m=m_cur, keep=keep, flags=flags, first=first)
        hc, hA, hb, hm = fm_host.step(fmlib, A_cur, b_cur, col, m=m_cur, keep=keep, flags=flags, first=first)
        assert np.array_equal(cnt, hc) and np.array_equal(mo, hm)
        assert np.array_equal(Ao, hA) and np.array_equal(bo, hb)   # bit for bit, zero padding included
        live = mo > 0
        assert live.all()
        res = pa.reduce_batch(Ao, bo, m=mo)
        checked = 0
        for t in range(0, B, 7 if family == "tulip" else 3):
            if mo[t] > 256:   # (the oracle's keep words cover 256 rows)
                continue
            o = oracle.reduce(Ao[t, :mo[t]], bo[t, :mo[t]])
            got = pa.keep_to_bool(res["keep"][t:t + 1], Ao.shape[1])[0, :mo[t]]
            assert np.array_equal(got, o["keep"]), t
            checked += 1
        assert checked > 50
        if family == "wide" and col == 4:
            assert Ao.shape[1] > 64 and (mo > 64).sum() > 100
        keep, flags = res["keep"], res["flags"]
        A_cur, b_cur, m_cur = Ao, bo, mo
        first = False


def mixed_batch(rng):
    """About 10 000 polytopes in d = 4, projected onto coordinates 1..3: ragged TuLiP shapes, outputs above 64 rows (the
    wide reduce), one polytope whose step forms more rows than the fused reduce takes (routed to the host), rows a hair
    apart, and the polytope of g23 (case 337) whose Chebyshev LP the fused reduce hands back (RF_F1OPEN: re-examined)."""
    from conftest import load_golden
    polys = []
    A, b = tulip_batch(rng, 9700, 3, 1, 8)
    polys += [(A[t], b[t]) for t in range(len(A))]
    for t in range(300):
        X, h = sphere(rng, 10 + t % 15, 4)
        polys.append((X, h))
    for t in range(40):
        X, h = sphere(rng, 24 + t % 8, 4)   # |P| |Q| ~ 150 rows after the step: the wide reduce
        polys.append((X, h))
    X, h = sphere(rng, 80, 4)                # ~1600 rows after the step: beyond the LDS reduce
    polys.append((X, h))
    for t in range(20):                      # rows a hair apart
        X, h = sphere(rng, 12, 4)
        polys.append((np.vstack([X, X[0]]), np.r_[h, h[0] + 1e-9]))
    polys.append((np.eye(4), np.ones(4)))    # (the slot of the g23 polytope)
    m_max = max(p[0].shape[0] for p in polys)
    B = len(polys)
    A = np.zeros((B, m_max, 4))
    b = np.zeros((B, m_max))
    m = np.zeros(B, np.int32)
    for t, (X, h) in enumerate(polys):
        P = pa.Polytope(X, h)
        A[t, :len(h)], b[t, :len(h)], m[t] = P.A, P.b, len(h)
    g = load_golden("g23_reduce_dup.npz")
    mm, dd = int(g["m"][337]), int(g["d"][337])
    assert dd == 4
    A[B - 1] = 0.0
    b[B - 1] = 0.0
    A[B - 1, :mm] = g["A"][337, :mm * dd].reshape(mm, dd)   # (as recorded: the rows are not normalised)
    b[B - 1, :mm] = g["b"][337, :mm]
    m[B - 1] = mm
    return A, b, m


def test_projection_batch_against_per_polytope(hip_backend):
    rng = np.random.default_rng(12)
    A, b, m = mixed_batch(rng)
    res = pa.projection_batch(A, b, [1, 2, 3], m=m)
    assert A.shape[0] >= 10000
    assert res["routed"] >= 1 and res["reexamined"] >= 1
    assert np.all(res["status"] <= 1)
    B = A.shape[0]
    sample = list(range(0, B, 25)) + list(range(B - 362, B))
    for t in sorted(set(sample)):
        P = pa.Polytope(A[t, :m[t]].copy(), b[t, :m[t]].copy(), normalize=False)
        Q = alg.projection(P, [1, 2, 3], solver="fm")
        if Q.A.size == 0:
            assert res["status"][t] == 1, t
            continue
        assert res["status"][t] == 0, t
        k = int(res["m"][t])
        assert np.array_equal(res["A"][t, :k], Q.A) and np.array_equal(res["b"][t, :k], Q.b), t


def test_projection_batch_device_tensors(hip_backend):
    import torch
    rng = np.random.default_rng(13)
    A, b = tulip_batch(rng, 300, 3, 1, 8)
    want = pa.projection_batch(A, b, [1, 2, 3])
    dev = torch.device("cuda:0")
    got = pa.projection_batch(torch.as_tensor(A, device=dev), torch.as_tensor(b, device=dev), [1, 2, 3])
    for key in ("A", "b", "m", "status"):
        assert got[key].is_cuda
        assert np.array_equal(got[key].cpu().numpy(), want[key])


def test_projection_batch_against_scipy_backend():
    """Independent of the device driver: the reference's algorithm restated on the scipy backend (np.dot combinations,
    HiGHS reductions) on a sample of the mixed batch -- the same sets, rows to 1e-7."""
    rng = np.random.default_rng(12)
    A, b, m = mixed_batch(rng)
    saved = solvers.default_solver
    solvers.default_solver = "hip"
    try:
        res = pa.projection_batch(A, b, [1, 2, 3], m=m)
    finally:
        solvers.default_solver = saved
    B = A.shape[0]
    # (not the g23 polytope, B - 1: its projection onto 1..3 is a strip that widens at the rate of its twin rows, 1e-9 --
    # the Chebyshev LP of that step is unbounded in exact arithmetic, HiGHS calls it optimal at r = 3 within its
    # tolerance, the engine's certified LP unbounded; the per-polytope test above holds it to projection() on 'hip')
    sample = list(range(0, 9700, 190)) + list(range(9700, B - 22, 9))
    solvers.default_solver = "scipy"
    try:
        for t in sample:
            Q = alg.projection(pa.Polytope(A[t, :m[t]].copy(), b[t, :m[t]].copy(), normalize=False), [1, 2, 3], solver="fm")
            if Q.A.size == 0:
                assert res["status"][t] == 1, t
                continue
            assert res["status"][t] == 0, t
            k = int(res["m"][t])
            want = np.c_[Q.A, Q.b]
            used = np.zeros(len(want), bool)
            assert k == len(want), (t, k, len(want))
            for row in np.c_[res["A"][t, :k], res["b"][t, :k]]:
                dist = np.abs(want - row).max(1)
                dist[used] = np.inf
                j = int(np.argmin(dist))
                assert dist[j] <= 1e-7, (t, row)
                used[j] = True
    finally:
        solvers.default_solver = saved


def test_projection_batch_minrep_inputs(hip_backend):
    """minrep=True: no first reduce, the rows as given go straight to the first elimination (after copy()'s pass)."""
    rng = np.random.default_rng(14)
    B = 500
    A = np.zeros((B, 8, 4))
    b = np.zeros((B, 8))
    for t in range(B):
        lo = -1 - rng.random(4)
        hi = 1 + rng.random(4)
        P = pa.Polytope.from_box(np.c_[lo, hi])
        A[t], b[t] = P.A, P.b
    res = pa.projection_batch(A, b, [1, 3], minrep=True)
    assert np.all(res["status"] == 0)
    for t in range(0, B, 10):
        P = pa.Polytope(A[t].copy(), b[t].copy(), minrep=True, normalize=False)
        Q = alg.projection(P, [1, 3], solver="fm")
        k = int(res["m"][t])
        assert np.array_equal(res["A"][t, :k], Q.A) and np.array_equal(res["b"][t, :k], Q.b), t


def test_regular_polygon_rows_vanish_in_the_step(hip_backend):
    """An 18-gon onto x: 66 candidate rows, 58 after the 8 antiparallel pairs vanish -- the keep words of the reduce must
    span the 66-row tensor they travel with.  Also a packed batch with 80 row slots and every polytope <= 64 rows."""
    t = np.deg2rad(np.arange(0, 360, 20))
    P = pa.Polytope(np.c_[np.cos(t), np.sin(t)], np.ones(18))
    Q = alg.projection(P, [1], solver="fm")
    order = np.argsort(Q.A[:, 0])
    assert np.allclose(Q.A[order, 0], [-1, 1], atol=1e-12) and np.allclose(Q.b[order], [1, 1], atol=1e-12)
    rng = np.random.default_rng(15)
    A = np.zeros((50, 80, 3))
    b = np.zeros((50, 80))
    ms = rng.integers(12, 65, 50).astype(np.int32)
    for k in range(50):
        X, h = sphere(rng, int(ms[k]), 3)
        A[k, :ms[k]], b[k, :ms[k]] = X, h
    res = pa.projection_batch(A, b, [1, 2], m=ms)
    for k in range(0, 50, 5):
        Q = alg.projection(pa.Polytope(A[k, :ms[k]].copy(), b[k, :ms[k]].copy(), normalize=False), [1, 2], solver="fm")
        n = int(res["m"][k])
        assert np.array_equal(res["A"][k, :n], Q.A) and np.array_equal(res["b"][k, :n], Q.b), k
