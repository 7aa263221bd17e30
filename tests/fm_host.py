"""Host build of polytope_amd/csrc/plp_fm.hpp (tests/cabi/fm_host.cpp, g++ -ffp-contract=off) and a numpy statement of
the Fourier-Motzkin step it implements, for tests/test_projection.py (CPU) and tests/test_projection_gpu.py (device rows
against the host, bit for bit)."""
import ctypes as C
import os
import subprocess
from fractions import Fraction

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build(tmpdir):
    out = os.path.join(str(tmpdir), "libfm_host.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-o", out,
                           os.path.join(ROOT, "tests", "cabi", "fm_host.cpp")])
    L = C.CDLL(out)
    L.fm_step.restype = C.c_int
    L.fm_step.argtypes = [C.c_longlong, C.c_int, C.c_int] + [C.c_void_p] * 4 + [C.c_int, C.c_void_p, C.c_int, C.c_int,
                                                                                  C.c_double, C.c_int] + [C.c_void_p] * 4
    return L


def _p(a):
    return None if a is None else C.c_void_p(a.ctypes.data)


def step(L, A, b, col, m=None, keep=None, flags=None, first=False, tol=1e-7, mo_max=None):
    """-> (count[B], A_out[B, mo, d'], b_out[B, mo], m_out[B]) with mo = mo_max, or max(count) without it, as
    plp_fm_count + plp_fm_emit."""
    A = np.ascontiguousarray(A, dtype=np.float64)
    B, m_max, d = A.shape
    b = np.ascontiguousarray(b, dtype=np.float64).reshape(B, m_max)
    m = None if m is None else np.ascontiguousarray(m, dtype=np.int32)
    kp = None if keep is None else np.ascontiguousarray(np.asarray(keep).astype(np.uint64).reshape(B, -1))
    kw = 0 if kp is None else kp.shape[1]
    fl = None if flags is None else np.ascontiguousarray(flags, dtype=np.int32)
    count = np.zeros(B, np.int32)
    rc = L.fm_step(B, m_max, d, _p(A), _p(b), _p(m), _p(kp), kw, _p(fl), int(col), int(first), tol, 0, _p(count),
                   None, None, None)
    assert rc == 0
    mo = max(int(count.max()) if B else 0, 1) if mo_max is None else int(mo_max)
    dout = d - 1 if col >= 0 else d
    Ao = np.zeros((B, mo, dout))
    bo = np.zeros((B, mo))
    mout = np.zeros(B, np.int32)
    rc = L.fm_step(B, m_max, d, _p(A), _p(b), _p(m), _p(kp), kw, _p(fl), int(col), int(first), tol, mo, None, _p(Ao),
                   _p(bo), _p(mout))
    assert rc == 0
    return count, Ao, bo, mout


# ---------------------------------------------------------------------------------------------- numpy statement
def fma(a, b, c):
    """a * b + c rounded once (exact rational arithmetic, correctly rounded by float())."""
    return float(Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c)))


def construct(A, b):
    """Polytope.__init__'s scaling (ref :130-138): rows of norm <= 1e-10 dropped, the rest times the reciprocal norm."""
    A = np.asarray(A, dtype=float)
    if A.shape[0] == 0:
        return A, np.asarray(b, dtype=float)
    nrm = np.sqrt(np.add.reduce(A * A, 1))
    rows = np.nonzero(nrm > 1e-10)[0]
    s = 1 / nrm[rows]
    return A[rows] * s[:, None], np.asarray(b, dtype=float)[rows] * s


def step_numpy(A, b, col, shift=False, passes=0, tol=1e-7):
    """One step on ONE polytope's rows (already compacted): the staging passes, the P / Q / N split, the combination
    fma(a_j, x_k, (-a_k) * x_j), column col removed, the constructor's scaling."""
    A = np.array(A, dtype=float)
    b = np.array(b, dtype=float)
    if shift:
        b = (b + 0.1) - 0.1
    for _ in range(passes):
        A, b = construct(A, b)
    a = A[:, col]
    P = np.nonzero(a > tol)[0]
    Q = np.nonzero(a < -tol)[0]
    N = np.nonzero(np.abs(a) < tol)[0]
    rows, rhs = [], []
    for j in P:
        for k in Q:
            rows.append([fma(A[j, col], A[k, c], -A[k, col] * A[j, c]) for c in range(A.shape[1])])
            rhs.append(fma(A[j, col], b[k], -A[k, col] * b[j]))
    for j in N:
        rows.append(list(A[j]))
        rhs.append(b[j])
    count = len(rows)
    Y = np.array(rows, dtype=float).reshape(count, A.shape[1]) if count else np.zeros((0, A.shape[1]))
    Y = np.delete(Y, col, axis=1)
    Y, yb = construct(Y, np.array(rhs, dtype=float))
    return count, Y, yb
