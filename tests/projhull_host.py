"""Host build of polytope_amd/csrc/plp_projhull.hpp (tests/cabi/projhull_host.cpp, g++ -ffp-contract=off) for
tests/test_projhull_host.py: the rule of projhull_kernel on the CPU, its LPs answered by a Python function -- and what the
CPU and GPU tests of projection_hull_batch share: the g31 fixture, packing, and the three checks that define "correct"."""
import ctypes as C
import os
import sys

import numpy as np

import host_build as hb

if hb.ROOT not in sys.path:
    sys.path.insert(0, hb.ROOT)
from oracle import oracle  # noqa: E402  (the C oracle, as conftest's fixture imports it)

SRC = os.path.join(hb.ROOT, "tests", "cabi", "projhull_host.cpp")
GOLDEN = os.path.join(hb.ROOT, "tests", "golden", "g31_projection_hull.npz")
(PH_OK, PH_UNBOUNDED, PH_FLAT, PH_OVERFLOW_POINTS, PH_OVERFLOW_FACETS, PH_BUDGET, PH_LPFAIL,
 PH_NOCENTRE) = range(8)   # plp::projhull::Status
MAX_POINTS, F_CAP = 64, 128
CONF_TOL = 1e-8
# Check (c): by how much a vertex of ours may violate a reference row beyond that case's ref_gap, on the frame of the case
# (lengths divided by `scale`).  Measured over the pinned cases of g31 with the host rule (test_projhull_host prints it):
# the worst excess was 1.45e-13 (the reference's rows on these cases hold its own vertices to rounding; HiGHS moves with
# its tolerances), so the bound is ten times that.
REF_MARGIN = 1.45e-12
_CB = C.CFUNCTYPE(C.c_int, C.c_longlong, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_int), C.POINTER(C.c_double), C.c_void_p)


def build(tmpdir):
    L = C.CDLL(hb.build(SRC, "libprojhull_host.so", tmpdir))
    vp, i, ll = C.c_void_p, C.c_int, C.c_longlong
    L.projhull_host.restype = i
    L.projhull_host.argtypes = [ll, i, i, i, vp, vp, vp, vp, vp, i, i, _CB, vp] + [vp] * 11
    return L


def build_program(tmpdir):
    """The stand-alone program (-DPROJHULL_HOST_MAIN) under -fsanitize=address,undefined -> its path."""
    return hb.build_program(SRC, "PROJHULL_HOST_MAIN", "projhull_host_san", tmpdir)


def upper_bound(k):
    """The upper-bound theorem for 64 points in R^k (written out again: the tests do not ask the code)."""
    return hb.upper_bound(k, MAX_POINTS)


def oracle_lp(A, b):
    """-> lp(c): max c.x over {A x <= b} by the oracle's certified LP -> (status, x or None)."""
    def lp(c):
        st, x, _, _ = oracle.lp_solve(-np.asarray(c, dtype=float), A, b)
        return st, x
    return lp


def centre(A, b):
    r, xc = oracle.cheby_ball(A, b)
    return None if xc is None or not r > 0 else np.asarray(xc, dtype=float)


def run(L, A, b, m, dim, xc, lp_of, f_max=None, max_lps=4096, points=True):
    """The rule on the packed batch A[B, m_max, d], b, m (None: m_max) onto the 1-based, increasing `dim`; lp_of(p, c) ->
    (status, x).  -> the dict of projection_hull_batch plus nrank[B] and asked: [(p, c)] in the order the rule asked."""
    A, b = np.ascontiguousarray(A, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    B, m_max, d = A.shape
    m = None if m is None else np.ascontiguousarray(m, dtype=np.int32)
    keep = np.ascontiguousarray(np.asarray(dim).ravel() - 1, dtype=np.int32)
    k = keep.size
    xc = np.ascontiguousarray(xc, dtype=np.float64).reshape(B, d)
    f_max = upper_bound(k) if f_max is None else f_max
    Ao, bo = np.full((B, f_max, k), 7.0), np.full((B, f_max), 7.0)
    on, count = np.full((B, f_max), 7, np.uint64), np.full(B, -1, np.int32)
    V, nv = np.full((B, MAX_POINTS, k), 7.0), np.full(B, -1, np.int32)
    X = np.full((B, MAX_POINTS, d), 7.0) if points else None
    vmask, nlp = np.full(B, 7, np.uint64), np.full(B, -1, np.int32)
    status, nrank = np.full(B, -1, np.int32), np.full(B, -1, np.int32)
    asked, raised = [], []

    def cb(p, dd, c, st_out, x_out, _user):
        try:
            cc = np.ctypeslib.as_array(c, shape=(dd,)).copy()
            asked.append((int(p), cc))
            st, x = lp_of(int(p), cc)
            st_out[0] = int(st)
            if st == 0:
                for t in range(dd):
                    x_out[t] = float(x[t])
            return 0
        except BaseException as e:   # (an exception cannot cross the C frames: end the call, raise it afterwards)
            raised.append(e)
            return 99
    rc = L.projhull_host(B, m_max, d, k, hb.ptr(A), hb.ptr(b), hb.ptr(m), hb.ptr(keep), hb.ptr(xc), f_max, max_lps, _CB(cb), None,
                         hb.ptr(Ao), hb.ptr(bo), hb.ptr(on), hb.ptr(count), hb.ptr(V), hb.ptr(nv), hb.ptr(X), hb.ptr(vmask),
                         hb.ptr(nlp), hb.ptr(status), hb.ptr(nrank))
    if raised:
        raise raised[0]
    assert rc == 0, rc
    res = dict(A=Ao, b=bo, on=on, m=count, V=V, nv=nv, vmask=vmask, nlp=nlp, status=status, nrank=nrank, asked=asked)
    if points:
        res["X"] = X
    return res


# ------------------------------------------------------------------------------------------------------------ the fixture
class Case(object):
    """One case of g31: family (a name), A[m, d], b[m], dim (1-based), expect (the PH_* status the rule must give),
    ref_kind (0: ref_A / ref_b / ref_V hold the reference's projection and its extreme(); 1: it returned Polytope(); 2: it
    raised; 3: not asked), ref_gap, pinned, reason."""


def load():
    z = np.load(GOLDEN)
    fams = [str(s) for s in z["families"]]
    out = []
    for i in range(len(z["family"])):
        c = Case()
        c.index, c.family = i, fams[int(z["family"][i])]
        d, m, k = int(z["d"][i]), int(z["m"][i]), int(z["k"][i])
        c.A = z["A"][z["a_off"][i]:z["a_off"][i + 1]].reshape(m, d)
        c.b = z["b"][z["b_off"][i]:z["b_off"][i + 1]]
        c.dim = z["dim"][z["dim_off"][i]:z["dim_off"][i + 1]].astype(np.int64)
        c.expect, c.ref_kind = int(z["expect"][i]), int(z["ref_kind"][i])
        c.ref_A = z["ref_A"][z["ra_off"][i]:z["ra_off"][i + 1]].reshape(-1, k)
        c.ref_b = z["ref_b"][z["rb_off"][i]:z["rb_off"][i + 1]]
        c.ref_V = z["ref_V"][z["rv_off"][i]:z["rv_off"][i + 1]].reshape(-1, k)
        c.ref_gap, c.pinned, c.reason = float(z["ref_gap"][i]), bool(z["pinned"][i]), int(z["reason"][i])
        out.append(c)
    return out


def pack(cases):
    """[(A, b)] of one d -> A[B, m_max, d], b[B, m_max], m[B] (NaN beyond m: nothing may read there)."""
    m = np.array([a.shape[0] for a, _ in cases], dtype=np.int32)
    d = cases[0][0].shape[1]
    A, b = np.full((len(cases), int(m.max()), d), np.nan), np.full((len(cases), int(m.max())), np.nan)
    for i, (a, bb) in enumerate(cases):
        A[i, :m[i]], b[i, :m[i]] = a, bb
    return A, b, m


# ------------------------------------------------------------------------------------------- what "correct" means
def scale_of(V):
    """The half-extent of the points' box: the frame every tolerance of the rule is absolute on."""
    return float(np.max((V.max(axis=0) - V.min(axis=0)) / 2.0))


def support(A, b, c):
    """max c.x over {A x <= b} by an LP that is not the code under test (the oracle's certified one)."""
    st, x, fun, _ = oracle.lp_solve(-np.asarray(c, dtype=float), A, b)
    assert st == 0, st
    return -fun


def lift(a, dim, d):
    c = np.zeros(d)
    c[np.asarray(dim) - 1] = a
    return c


def check_outer(A, b, dim, Ao, bo, s, support_of=support):
    """(a) every output row holds the whole polytope: its support value is at most bo + 2 CONF_TOL s.  -> the worst excess
    over bo, in units of s."""
    worst = -np.inf
    for a, bb in zip(Ao, bo):
        assert abs(np.linalg.norm(a) - 1.0) <= 1e-12
        h = support_of(A, b, lift(a, dim, A.shape[1]))
        worst = max(worst, (h - bb) / s)
        assert h <= bb + 2 * CONF_TOL * s, (h, bb, s)
    return worst


def check_inner(A, b, dim, V, X):
    """(b) every X row is a point of the polytope (to 1e-9 max(1, |b|_max)) whose kept coordinates are the V row."""
    tol = 1e-9 * max(1.0, float(np.max(np.abs(b))))
    assert np.all(np.isfinite(X)) and np.all(np.isfinite(V))
    assert np.max(X @ A.T - b[None, :]) <= tol
    assert np.array_equal(X[:, np.asarray(dim) - 1], V)


def check_reference(case, Ao, bo, V, vmask, s):
    """(c) the reference's vertices satisfy our rows to the tolerance of (a) plus ref_gap; our vmask vertices violate a
    reference row by at most ref_gap plus REF_MARGIN s.  -> the worst excess of the second over ref_gap, in units of s."""
    assert np.max(case.ref_V @ Ao.T - bo[None, :]) <= 2 * CONF_TOL * s + case.ref_gap
    mine = V[[i for i in range(V.shape[0]) if (int(vmask) >> i) & 1]]
    assert mine.shape[0] >= V.shape[1] + 1 or V.shape[1] == 1 and mine.shape[0] == 2
    nrm = np.linalg.norm(case.ref_A, axis=1)
    over = np.max((mine @ case.ref_A.T - case.ref_b[None, :]) / nrm[None, :]) - case.ref_gap
    assert over <= REF_MARGIN * s, (over, s)
    return over / s


def check_all(case, res, p, support_of=support):
    """(a), (b), (c) on member p of a result of run() / projection_hull_batch (numpy) for a case that expects PH_OK ->
    (worst outer excess, worst reference excess) in units of the frame."""
    cnt, nv = int(res["m"][p]), int(res["nv"][p])
    Ao, bo, V = res["A"][p, :cnt], res["b"][p, :cnt], res["V"][p, :nv]
    assert cnt >= len(case.dim) + 1 or len(case.dim) == 1 and cnt == 2
    assert np.all(np.isnan(res["A"][p, cnt:])) and np.all(np.isnan(res["b"][p, cnt:])) and np.all(np.isnan(res["V"][p, nv:]))
    s = scale_of(V)
    outer = check_outer(case.A, case.b, case.dim, Ao, bo, s, support_of)
    if "X" in res:
        check_inner(case.A, case.b, case.dim, V, res["X"][p, :nv])
    ref = check_reference(case, Ao, bo, V, res["vmask"][p], s) if case.ref_kind == 0 else -np.inf
    return outer, ref
