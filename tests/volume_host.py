"""Host build of polytope_amd/csrc/plp_volume.hpp (tests/cabi/volume_host.cpp, g++ -ffp-contract=off) for
tests/test_volume_host.py (CPU: the stream against numpy, the hit counts against the reference's) and
tests/test_volume_gpu.py (device hit counts against the host, bit for bit)."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build(tmpdir):
    out = os.path.join(str(tmpdir), "libvolume_host.so")
    # -fopenmp: vh_hits spreads the polytopes of a batch over the cores (each polytope is still one sequential loop)
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fopenmp", "-fPIC", "-shared", "-o", out,
                           os.path.join(ROOT, "tests", "cabi", "volume_host.cpp")])
    L = C.CDLL(out)
    L.vh_stream.restype = None
    L.vh_stream.argtypes = [C.c_void_p, C.c_void_p, C.c_longlong, C.c_void_p]
    L.vh_advance.restype = None
    L.vh_advance.argtypes = [C.c_void_p, C.c_void_p, C.c_longlong, C.c_void_p, C.c_int, C.c_void_p]
    L.vh_at.restype = None
    L.vh_at.argtypes = [C.c_void_p, C.c_void_p, C.c_longlong, C.c_void_p, C.c_void_p]
    L.vh_hits.restype = C.c_int
    L.vh_hits.argtypes = [C.c_longlong, C.c_int, C.c_int] + [C.c_void_p] * 7 + [C.c_longlong, C.c_void_p, C.c_void_p]
    return L


def _p(a):
    return None if a is None else C.c_void_p(a.ctypes.data)


def words(v):
    """128-bit integer -> uint64[2], low word first."""
    return np.array([v & 0xFFFFFFFFFFFFFFFF, v >> 64], dtype=np.uint64)


def seed_state(seed):
    """(state[2], inc[2]) of np.random.PCG64(seed), the generator default_rng(seed) uses."""
    st = np.random.PCG64(seed).state["state"]
    return words(st["state"]), words(st["inc"])


def stream(L, seed, count):
    s, i = seed_state(seed)
    out = np.empty(count)
    L.vh_stream(_p(s), _p(i), count, _p(out))
    return out


def advance(L, seed, n, jump=False):
    """States (as Python ints) after n[i] steps from the seed's initial state."""
    s, i = seed_state(seed)
    n = np.ascontiguousarray(n, dtype=np.uint64)
    out = np.empty((n.size, 2), np.uint64)
    L.vh_advance(_p(s), _p(i), n.size, _p(n), int(jump), _p(out))
    return [int(lo) | (int(hi) << 64) for lo, hi in out]


def at(L, seed, pos):
    s, i = seed_state(seed)
    pos = np.ascontiguousarray(pos, dtype=np.uint64)
    out = np.empty(pos.size)
    L.vh_at(_p(s), _p(i), pos.size, _p(pos), _p(out))
    return out


def hits(L, A, b, lb, ub, state, inc, N, m=None):
    """-> (hits uint32[B], flags int32[B]) as plp_volume_hits."""
    A = np.ascontiguousarray(A, dtype=np.float64)
    B, m_max, d = A.shape
    b = np.ascontiguousarray(b, dtype=np.float64).reshape(B, m_max)
    lb = np.ascontiguousarray(lb, dtype=np.float64).reshape(B, d)
    ub = np.ascontiguousarray(ub, dtype=np.float64).reshape(B, d)
    state = np.ascontiguousarray(state, dtype=np.uint64).reshape(B, 2)
    inc = np.ascontiguousarray(inc, dtype=np.uint64).reshape(B, 2)
    m = None if m is None else np.ascontiguousarray(m, dtype=np.int32)
    h = np.zeros(B, np.uint32)
    fl = np.zeros(B, np.int32)
    rc = L.vh_hits(B, m_max, d, _p(A), _p(b), _p(m), _p(lb), _p(ub), _p(state), _p(inc), int(N), _p(h), _p(fl))
    assert rc == 0
    return h, fl
