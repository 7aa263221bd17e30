"""CPU: projection() and its helpers (polytope_amd/polytope.py; reference polytope/polytope.py:1698-2114) on the scipy
backend against the reference's answers (tests/golden/g27_projection.npz, make_golden_projection.py), the reference's
quirks kept on purpose, and the row arithmetic of the Fourier-Motzkin step kernels (csrc/plp_fm.hpp, built for the host
by tests/cabi/fm_host.cpp) against a numpy statement of the chosen combination formula."""
import logging
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import polytope_amd as pa  # noqa: E402
from polytope_amd import solvers  # noqa: E402
from polytope_amd import polytope as alg  # noqa: E402
from conftest import load_golden  # noqa: E402
import fm_host  # noqa: E402

SOLVERS = ["fm", "exthull", "iterhull", "none", "bogus", "fm_direct"]


def g27_cases():
    g = load_golden("g27_projection.npz")
    out = []
    va = vo = 0   # offsets into the flat value arrays (rows x columns of the cases before)
    for k in range(len(g["kind"])):
        d = int(g["in_d"][k])
        lo, hi = g["in_off"][k], g["in_off"][k + 1]
        olo, ohi = g["out_off"][k], g["out_off"][k + 1]
        od = int(g["out_dim"][k])
        A = g["in_A"][va:va + (hi - lo) * d].reshape(-1, d)
        QA = g["out_A"][vo:vo + (ohi - olo) * od].reshape(-1, od)
        va += (hi - lo) * d
        vo += (ohi - olo) * od
        out.append(dict(
            kind=str(g["kind"][k]), solver=SOLVERS[int(g["solver"][k])], seed=int(g["seed"][k]), tie=bool(g["tie"][k]),
            minrep=bool(g["minrep"][k]), A=A, b=g["in_b"][lo:hi],
            dim=[int(v) for v in g["dim"][g["dim_off"][k]:g["dim_off"][k + 1]]], status=int(g["status"][k]),
            QA=QA, Qb=g["out_b"][olo:ohi]))
    return out


def run_case(c):
    """(status, A, b) of this package's projection on case c (status as in the fixture)."""
    P = pa.Polytope(c["A"].copy(), c["b"].copy(), minrep=c["minrep"])
    np.random.seed(c["seed"])
    try:
        if c["solver"] == "fm_direct":
            d = c["A"].shape[1]
            Q = alg.projection_fm(P, None, np.setdiff1d(range(d), np.array(c["dim"]) - 1))
        else:
            Q = alg.projection(P, c["dim"], solver=None if c["solver"] == "none" else c["solver"])
    except IndexError:
        return 2, None, None
    if Q.A.size == 0:
        return 1, None, None
    return 0, Q.A, Q.b


def check_case(c, got):
    st, A, b = got
    assert st == c["status"], (c["kind"], st, c["status"])
    if st != 0:
        return
    QA, Qb = c["QA"], c["Qb"]
    assert A.shape == QA.shape, (c["kind"], A.shape, QA.shape)
    if not c["tie"]:
        # Fourier-Motzkin without ties: the same rows in the same order
        assert np.allclose(A, QA, rtol=0, atol=1e-9) and np.allclose(b, Qb, rtol=0, atol=1e-9), c["kind"]
        return
    want = np.c_[QA, Qb]
    have = np.c_[A, b]
    used = np.zeros(len(want), bool)
    for row in have:
        d = np.abs(want - row).max(1)
        d[used] = np.inf
        j = int(np.argmin(d))
        assert d[j] <= 1e-7, (c["kind"], row, want)
        used[j] = True


@pytest.fixture(scope="module")
def fmlib(tmp_path_factory):
    return fm_host.build(tmp_path_factory.mktemp("fm"))


@pytest.fixture
def scipy_backend():
    saved = solvers.default_solver
    solvers.default_solver = "scipy"
    yield
    solvers.default_solver = saved


def test_g27_scipy(scipy_backend):
    cases = g27_cases()
    assert len(cases) > 100
    for c in cases:
        check_case(c, run_case(c))


def test_project_method_and_module_path(scipy_backend):
    P = pa.Polytope.from_box([[0, 1], [0, 2], [-1, 1]])
    Q = P.project([1, 2])
    assert Q.A.shape[1] == 2
    assert np.allclose(sorted(Q.b), sorted([1, 2, 0, 0]))
    assert alg.projection is pa.polytope.projection
    assert not hasattr(pa, "projection")   # the reference's module path only


def test_fm_direct_as_reference_tests_call_it(scipy_backend):
    a = np.array([[-1.0, 0.0], [1.0, 0.0], [0.0, -1.0], [0.0, 1.0]])
    P = pa.Polytope(a, np.array([-1.0, 2.0, -1.0, 2.0]))
    Q = alg.projection_fm(P, None, np.array([1]))
    order = np.argsort(Q.A, axis=0).flatten()
    assert np.allclose(Q.A[order], [[-1.0], [1.0]]) and np.allclose(Q.b[order], [-1.0, 2.0])


def test_fewer_rows_mutates_caller(scipy_backend):
    P = pa.Polytope(np.array([[1.0, 0, 0], [0, 1, 0]]), np.array([1.0, 1.0]))
    Q = alg.projection(P, [1, 2])
    assert P.A.shape == (3, 3) and np.array_equal(P.A[2], np.zeros(3)) and P.b.shape == (3,)
    assert Q.A.size == 0   # unbounded: the existence LP fails


def test_region_input_raises_typeerror(scipy_backend):
    P = pa.Polytope.from_box([[0, 1], [0, 1], [0, 1]])
    with pytest.raises(TypeError):
        alg.projection(pa.Region([P, P.translation([2, 0, 0])]), [1, 2])


def test_esp_raises(scipy_backend):
    P = pa.Polytope.from_box([[0, 1], [0, 1], [0, 1]])
    with pytest.raises(Exception, match="cvxopt.glpk"):
        alg.projection(P, [1, 2], solver="esp")


def test_unknown_solver_warns(scipy_backend, caplog):
    P = pa.Polytope.from_box([[0, 1], [0, 1], [0, 1]])
    with caplog.at_level(logging.WARNING):
        Q = alg.projection(P, [1, 2], solver="nonsense")
    assert "unrecognized projection solver" in caplog.text
    assert Q.A.shape == (4, 2)


def test_coefficient_split_at_abs_tol(scipy_backend, fmlib):
    # a coefficient of exactly +-abs_tol is in none of P / Q / N: its row is dropped (ref :1925-1927)
    tol = alg.ABS_TOL
    A = np.array([[1.0, 0.5], [-1.0, 0.5], [tol, 1.0], [0.0, -1.0], [-tol, 1.0]])
    P = pa.Polytope(A, np.array([1.0, 1.0, 5.0, 1.0, 5.0]), minrep=True)
    P.A = A.copy()   # the rows exactly as written (no scaling), as a reduced polytope would hold them
    P.b = np.array([1.0, 1.0, 5.0, 1.0, 5.0])
    poly = alg._fm_combine_host(P, 0)
    assert poly.A.shape[0] == 1 + 1   # P x Q = 1, N = {row 3}; rows 2 and 4 (+-tol) dropped
    cnt, Ao, bo, mo = fm_host.step(fmlib, A[None], np.array([[1.0, 1.0, 5.0, 1.0, 5.0]]), 0)
    assert int(cnt[0]) == 2 and int(mo[0]) == 2


def test_fm_host_against_numpy_statement(fmlib):
    rng = np.random.default_rng(5)
    for d in (2, 3, 4, 6, 9):
        B, m = 40, 12
        A = rng.standard_normal((B, m, d))
        b = rng.random((B, m)) + 0.5
        A[0, 3, :] = 0.0                                   # a zero row: dropped by the constructor pass
        A[1, 2, d - 1] = 1e-7                              # exactly +-abs_tol: in no list
        A[1, 5, d - 1] = -1e-7
        A[2, :, d - 1] = np.abs(A[2, :, d - 1])            # Q empty: only N rows survive
        ms = rng.integers(1, m + 1, B).astype(np.int32)
        keep = rng.integers(0, 1 << 12, B).astype(np.uint64)
        flags = rng.choice([2, 4], B).astype(np.int32)
        for col in (0, d - 1):
            for first in (False, True):
                cnt, Ao, bo, mo = fm_host.step(fmlib, A, b, col, m=ms, keep=keep, flags=flags, first=first)
                for k in range(B):
                    rows = [r for r in range(ms[k]) if (int(keep[k]) >> r) & 1]
                    c, Y, yb = fm_host.step_numpy(A[k, rows], b[k, rows], col, shift=bool(flags[k] & 4),
                                                  passes=1 + int(first))
                    assert int(cnt[k]) == c, (d, col, k)
                    assert int(mo[k]) == Y.shape[0]
                    assert np.array_equal(Ao[k, :mo[k]], Y) and np.array_equal(bo[k, :mo[k]], yb), (d, col, k)


def test_fm_host_compaction_only(fmlib):
    rng = np.random.default_rng(6)
    A = rng.standard_normal((10, 7, 3))
    b = rng.random((10, 7))
    cnt, Ao, bo, mo = fm_host.step(fmlib, A, b, -1, flags=np.full(10, 4, np.int32))
    for k in range(10):
        Y, yb = fm_host.construct(A[k], (b[k] + 0.1) - 0.1)
        assert np.array_equal(Ao[k, :mo[k]], Y) and np.array_equal(bo[k, :mo[k]], yb)


# ------------------------------------------------------------------------- the driver's shapes, without a device
class _HostEngine:
    """batch.fm_count / fm_emit / reduce_batch on the host for torch CPU tensors: the step kernels through their host build,
    the fused reduce through the oracle, and the step kernels' argument check (include/plp.h: kw >= ceil(m_max / 64))."""

    def __init__(self, fmlib, oracle):
        self.L, self.O = fmlib, oracle

    @staticmethod
    def _np(t):
        return None if t is None else t.cpu().numpy()

    def _check(self, A, keep):
        if keep is not None:
            assert keep.reshape(keep.shape[0], -1).shape[1] >= (A.shape[1] + 63) // 64, "keep words narrower than the rows"

    def fm_count(self, A, b, col, m=None, keep=None, flags=None, first=False, abs_tol=1e-7):
        import torch
        self._check(A, keep)
        cnt = fm_host.step(self.L, self._np(A), self._np(b), col, m=self._np(m), keep=self._np(keep), flags=self._np(flags),
                           first=first, tol=abs_tol)[0]
        return torch.as_tensor(cnt)

    def fm_emit(self, A, b, col, mo_max, m=None, keep=None, flags=None, first=False, abs_tol=1e-7):
        import torch
        self._check(A, keep)
        _, Ao, bo, mo = fm_host.step(self.L, self._np(A), self._np(b), col, m=self._np(m), keep=self._np(keep),
                                     flags=self._np(flags), first=first, tol=abs_tol, mo_max=mo_max)
        return torch.as_tensor(Ao), torch.as_tensor(bo), torch.as_tensor(mo)

    def reduce_batch(self, A, b, m=None, abs_tol=1e-7):
        import torch
        A, b = self._np(A), self._np(b)
        m = np.full(A.shape[0], A.shape[1]) if m is None else self._np(m)
        W = (A.shape[1] + 63) // 64
        keep = np.zeros((A.shape[0], W), np.uint64)
        flags = np.zeros(A.shape[0], np.int32)
        for k in range(A.shape[0]):
            o = self.O.reduce(A[k, :m[k]], b[k, :m[k]], abs_tol)
            keep[k] = np.array(o["words"][:W], np.uint64)
            flags[k] = o["flags"]
        keep = keep.view(np.int64)
        return dict(keep=torch.as_tensor(keep if W > 1 else keep[:, 0].copy()), flags=torch.as_tensor(flags))


def _drive(monkeypatch, fmlib, oracle, A, b, m, cols):
    import torch
    from polytope_amd import batch
    eng = _HostEngine(fmlib, oracle)
    for name in ("fm_count", "fm_emit", "reduce_batch"):
        monkeypatch.setattr(batch, name, getattr(eng, name))
    host = {}
    res = batch._fm_batch(torch.as_tensor(A), torch.as_tensor(b), torch.as_tensor(np.asarray(m, np.int32)), cols, 1e-7,
                          [False] * A.shape[0], lambda k, *a: host.setdefault(k, a))
    return res, host


def _same_set(A, b, QA, Qb, tol=1e-7):
    assert A.shape == QA.shape, (A.shape, QA.shape)
    want = np.c_[QA, Qb]
    used = np.zeros(len(want), bool)
    for row in np.c_[A, b]:
        dist = np.abs(want - row).max(1)
        dist[used] = np.inf
        j = int(np.argmin(dist))
        assert dist[j] <= tol, (row, want)
        used[j] = True


def test_driver_keep_words_follow_the_rows(monkeypatch, fmlib, oracle, scipy_backend):
    # a regular 18-gon onto x: 8 P rows, 8 Q rows and 2 N rows form 66 candidate rows; the 8 antiparallel pairs vanish
    # (norm 0), so 58 rows reach the reduce.  The keep words it returns travel with the 66-row tensor to the next call.
    t = np.deg2rad(np.arange(0, 360, 20))
    A = np.c_[np.cos(t), np.sin(t)]
    b = np.ones(18)
    res, host = _drive(monkeypatch, fmlib, oracle, A[None], b[None], [18], [1])
    assert not host
    idx, Ao, bo, mo, _ = res[-1]
    Q = alg.projection(pa.Polytope(A, b), [1], solver="fm")
    _same_set(Ao[0, :mo[0]], bo[0, :mo[0]], Q.A, Q.b, 1e-9)
    # a packed batch whose row slots (80) exceed every row count in use (<= 64): two keep words from the first step on
    rng = np.random.default_rng(3)
    B, slots = 6, 80
    A3 = np.zeros((B, slots, 3))
    b3 = np.zeros((B, slots))
    ms = []
    for k in range(B):
        X = rng.standard_normal((20 + 7 * k, 3))
        P = pa.Polytope(X, np.ones(len(X)))
        A3[k, :len(X)], b3[k, :len(X)] = P.A, P.b
        ms.append(len(X))
    res, host = _drive(monkeypatch, fmlib, oracle, A3, b3, ms, [2])
    idx, Ao, bo, mo, _ = res[-1]
    assert list(idx) == list(range(B)) and not host
    for k in range(B):
        Q = alg.projection_fm(pa.Polytope(A3[k, :ms[k]], b3[k, :ms[k]], normalize=False), None, np.array([2]))
        _same_set(Ao[k, :mo[k]], bo[k, :mo[k]], Q.A, Q.b)
