"""Host build of polytope_amd/csrc/plp_support.hpp (tests/cabi/support_host.cpp, g++ -ffp-contract=off) and the inputs
tests/test_support_host.py (CPU: the per-LP function against the oracle's simplex) and tests/test_support_gpu.py (device
answers against the host build bit for bit, and against the oracle) share: families, seeds, directions, oracle answers."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (m_max, d) of the random families; the seed of family k is SEED0 + k (kept here: the GPU tests reuse them)
SHAPES = ((5, 1), (7, 2), (16, 3), (17, 3), (33, 4), (64, 4))
SEED0 = 4100
B_FAMILY = 40
K_RANDOM = 9
HANDBACK_CAP = 0.01   # raw status 1 on the random bounded family, as a share of its LPs


def build(tmpdir):
    out = os.path.join(str(tmpdir), "libsupport_host.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-o", out,
                           os.path.join(ROOT, "tests", "cabi", "support_host.cpp")])
    L = C.CDLL(out)
    L.support_host.restype = C.c_int
    L.support_host.argtypes = [C.c_longlong, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p,
                               C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.support_polytopes_per_group.restype = C.c_int
    L.support_polytopes_per_group.argtypes = [C.c_int, C.c_int]
    return L


def _p(a):
    return None if a is None else C.c_void_p(a.ctypes.data)


def run(L, A, b, C_, xc, m=None, points=True):
    """plp_support_batch on the host -> (h[B, K], x[B, K, d] or None, status[B, K]), raw statuses."""
    A = np.ascontiguousarray(A, dtype=np.float64)
    B, m_max, d = A.shape
    b = np.ascontiguousarray(b, dtype=np.float64).reshape(B, m_max)
    C_ = np.ascontiguousarray(C_, dtype=np.float64)
    K = C_.shape[-2]
    xc = np.ascontiguousarray(xc, dtype=np.float64).reshape(B, d)
    m = None if m is None else np.ascontiguousarray(m, dtype=np.int32)
    h = np.empty((B, K))
    x = np.empty((B, K, d)) if points else None
    st = np.empty((B, K), np.int32)
    rc = L.support_host(B, m_max, d, _p(A), _p(b), _p(m), K, _p(C_), 1 if C_.ndim == 2 else 0, _p(xc), _p(h), _p(x), _p(st))
    assert rc == 0
    return h, x, st


def family(k, B=B_FAMILY, bounded=True, ragged=True):
    """Family k of SHAPES: random_hpolytopes with ragged row counts (rows beyond m[p] zeroed) -> A, b, m."""
    from polytope_amd.synth import random_hpolytopes
    m_max, d = SHAPES[k]
    A, b = random_hpolytopes(B, m_max, d, seed=SEED0 + k, bounded=bounded)
    m = np.full(B, m_max, np.int32)
    if ragged:
        lo = min(m_max, 2 * d if bounded else 1)
        m = np.random.default_rng(SEED0 + 100 + k).integers(lo, m_max + 1, size=B).astype(np.int32)
        m[0] = m_max
        for p in range(B):
            A[p, m[p]:] = 0.0
            b[p, m[p]:] = 0.0
    return A, b, m


def directions(k, B, shared, K=K_RANDOM, axes=True):
    """K random directions plus +-e_i: [K + 2 d, d] shared, or [B, K + 2 d, d]."""
    d = SHAPES[k][1]
    rng = np.random.default_rng(SEED0 + 200 + k + (50 if shared else 0))
    R = rng.standard_normal((K, d) if shared else (B, K, d))
    if not axes:
        return R
    E = np.vstack([np.eye(d), -np.eye(d)])
    return np.vstack([R, E]) if shared else np.concatenate([R, np.broadcast_to(E, (B, 2 * d, d))], axis=1)


def centres(O, A, b, m):
    """Chebyshev centres by the oracle (every polytope of the families has one)."""
    xc = np.zeros((A.shape[0], A.shape[2]))
    for p in range(A.shape[0]):
        st, r, c = O.cheby(A[p, :m[p]], b[p, :m[p]])
        assert st == 0 and r > 0
        xc[p] = c
    return xc


def oracle_support(O, A, b, m, C_):
    """(status[B, K], h[B, K]) by the oracle's simplex: min -c.x; h = -fun where the status is 0, NaN elsewhere."""
    B = A.shape[0]
    K = C_.shape[-2]
    st = np.zeros((B, K), np.int32)
    h = np.full((B, K), np.nan)
    for p in range(B):
        mp = A.shape[1] if m is None else int(m[p])
        for j in range(K):
            c = C_[j] if C_.ndim == 2 else C_[p, j]
            s, _, fun, _ = O.lp_solve(-c, A[p, :mp], b[p, :mp])
            st[p, j] = s
            if s == 0:
                h[p, j] = -fun
    return st, h


def check_against_oracle(A, b, m, C_, h, x, st, ost, oh, where=None):
    """The tolerance of the support tests: status equal to the oracle's; where it is 0, |h - h_oracle| <= 1e-9 max(1, |h|),
    A x <= b + 1e-9 and |c.x - h| <= 1e-12 max(1, |h|).  `where`: the LPs to look at (default: all)."""
    sel = np.ones(st.shape, bool) if where is None else where
    assert np.array_equal(st[sel], ost[sel]), np.argwhere(sel & (st != ost))[:5]
    ok = sel & (st == 0)
    assert np.all(np.abs(h[ok] - oh[ok]) <= 1e-9 * np.maximum(1.0, np.abs(h[ok]))), np.abs(h[ok] - oh[ok]).max()
    if x is None:
        return
    B, K = st.shape
    Cb = np.broadcast_to(C_, (B,) + C_.shape) if C_.ndim == 2 else C_
    cx = np.einsum("pjk,pjk->pj", Cb, x)
    assert np.all(np.abs(cx[ok] - h[ok]) <= 1e-12 * np.maximum(1.0, np.abs(h[ok])))
    Ax = np.einsum("pik,pjk->pji", A, x)   # [B, K, m_max]
    rows = np.arange(A.shape[1])[None, None, :] < (np.full(B, A.shape[1]) if m is None else m)[:, None, None]
    viol = np.where(rows, Ax - b[:, None, :], -np.inf).max(axis=2)
    assert np.all(viol[ok] <= 1e-9), viol[ok].max()


@functools.lru_cache(maxsize=None)
def _cached(key):
    return {}


def memo(key, make):
    """One value per key for the whole test session (oracle answers are computed once and shared)."""
    slot = _cached(key)
    if "v" not in slot:
        slot["v"] = make()
    return slot["v"]
