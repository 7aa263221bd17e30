"""Host build of polytope_amd/csrc/plp_pair_stack.hpp (tests/cabi/pair_stack_host.cpp, g++ -ffp-contract=off) for
tests/test_pair_stack_host.py (CPU: the header against numpy's constructor, bit for bit) and
tests/test_intersect_pairs_gpu.py (the device kernel against the host build and numpy); the numpy statement of the stack
rule and the seeded tables both files run."""
import ctypes as C
import os

import numpy as np

import host_build as hb

SRC = os.path.join(hb.ROOT, "tests", "cabi", "pair_stack_host.cpp")
M_MAXES = (4, 16, 32)
DIMS = tuple(range(1, 17))


def build(tmpdir):
    L = C.CDLL(hb.build(SRC, "libpair_stack_host.so", tmpdir))
    vp, i, ll = C.c_void_p, C.c_int, C.c_longlong
    L.psh_first_bad.restype = ll
    L.psh_first_bad.argtypes = [i, ll, vp]
    for fn in (L.psh_stacks, L.psh_stacks_unchecked):
        fn.restype = i
        fn.argtypes = [i, i, i, vp, vp, vp, ll, vp, vp, vp, vp]
    return L


def build_program(tmpdir):
    """The stand-alone program (-DPAIR_STACK_HOST_MAIN) under -fsanitize=address,undefined -> its path."""
    return hb.build_program(SRC, "PAIR_STACK_HOST_MAIN", "pair_stack_host_san", tmpdir)


def stacks(L, A, b, m, pairs, checked=True):
    """The host build on the table A[n, m_max, d], b, m (or None) -> (rc, A_s[K, 2 m_max, d], b_s[K, 2 m_max], m_s[K]);
    the outputs start as -7 everywhere, so a slot the build leaves unwritten shows."""
    A, b = np.ascontiguousarray(A, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    m = None if m is None else np.ascontiguousarray(m, dtype=np.int32)
    pairs = np.ascontiguousarray(pairs, dtype=np.int32).reshape(-1, 2)
    n, m_max, d = A.shape
    K = pairs.shape[0]
    A_s, b_s, m_s = np.full((K, 2 * m_max, d), -7.0), np.full((K, 2 * m_max), -7.0), np.full(K, -7, np.int32)
    fn = L.psh_stacks if checked else L.psh_stacks_unchecked
    rc = fn(n, m_max, d, hb.ptr(A), hb.ptr(b), hb.ptr(m), K, hb.ptr(pairs), hb.ptr(A_s), hb.ptr(b_s), hb.ptr(m_s))
    return rc, A_s, b_s, m_s


def numpy_stack(Ai, bi, Aj, bj):
    """What Polytope(np.vstack([A_i, A_j]), np.hstack([b_i, b_j])) holds (reference polytope.py:130-138, :272-275), written
    out with the reference's own numpy expressions -> (A, b)."""
    A, b = np.vstack([Ai, Aj]), np.hstack([bi, bj])
    if A.size == 0:
        return A.reshape(0, Ai.shape[1]), b
    norm = np.sqrt(np.sum(A * A, 1)).flatten()
    pos = np.nonzero(norm > 1e-10)[0]
    A, b, norm = A[pos, :], b[pos], norm[pos]
    inv = 1 / norm
    return A * inv[:, None], b.flatten() * inv


def numpy_stacks(A, b, m, pairs):
    """numpy_stack per listed pair, packed as the library packs -> A_s, b_s, m_s."""
    n, m_max, d = A.shape
    pairs = np.asarray(pairs).reshape(-1, 2)
    K, W = pairs.shape[0], 2 * m_max
    A_s, b_s, m_s = np.zeros((K, W, d)), np.zeros((K, W)), np.zeros(K, np.int32)
    mm = np.full(n, m_max) if m is None else m
    for t, (i, j) in enumerate(pairs):
        a, bb = numpy_stack(A[i, :mm[i]], b[i, :mm[i]], A[j, :mm[j]], b[j, :mm[j]])
        m_s[t] = a.shape[0]
        A_s[t, :a.shape[0]], b_s[t, :a.shape[0]] = a, bb
    return A_s, b_s, m_s


def table(d, m_max, seed=0, n=7, pad=np.nan):
    """n = 7 cells in dimension d with ragged row counts 1..m_max (cell 0 has m_max rows, cell 1 one row): random rows
    scaled by 1e-3 .. 30, one row of norm 1e-11 and one all-zero row (both are dropped, the rows behind them move up);
    everything at and beyond row m[p] is `pad` (NaN: reading it would show) -> A[n, m_max, d], b[n, m_max], m[n]."""
    rng = np.random.default_rng(1000 * d + m_max + 7919 * seed)
    m = rng.integers(1, m_max + 1, n).astype(np.int32)
    m[0], m[1] = m_max, 1
    A, b = np.full((n, m_max, d), pad), np.full((n, m_max), pad)
    for p in range(n):
        rows = rng.standard_normal((m[p], d))
        rows /= np.linalg.norm(rows, axis=1, keepdims=True)
        scale = 10.0 ** rng.uniform(-3, np.log10(30.0), m[p])
        A[p, :m[p]] = rows * scale[:, None]
        b[p, :m[p]] = rng.uniform(0.5, 2.0, m[p]) * scale
    # the dropped rows: a tiny one in the middle of cell 0 (rows behind it move up), a zero row first in cell 2, and a
    # tiny LAST row in cell 3 when it has more than one
    A[0, m_max // 2] *= 1e-11 / np.linalg.norm(A[0, m_max // 2])
    A[2, 0] = 0.0
    if m[3] > 1:
        A[3, m[3] - 1] *= 1e-11 / np.linalg.norm(A[3, m[3] - 1])
    return A, b, m


def all_pairs(n=7):
    """The n (n - 1) ordered pairs -- (i, j) and (j, i) both occur -- and three repeats."""
    p = [(i, j) for i in range(n) for j in range(n) if i != j]
    return np.array(p + [p[0], p[5], p[0]], dtype=np.int32)


BAD_PAIRS = ((-1, 2), (2, -1), (7, 0), (0, 7), (3, 3), (2 ** 31 - 1, 0), (-2 ** 31, 1))


def write_cases(path, cases):
    """The stand-alone program's input: cases = [(A, b, m, pairs, A_s, b_s, m_s)]."""
    with open(path, "wb") as f:
        f.write(np.int64(len(cases)).tobytes())
        for A, b, m, pairs, A_s, b_s, m_s in cases:
            n, m_max, d = A.shape
            f.write(np.array([n, m_max, d, len(pairs)], np.int64).tobytes())
            for a, dt in ((A, np.float64), (b, np.float64), (m, np.int32), (pairs, np.int32), (A_s, np.float64),
                          (b_s, np.float64), (m_s, np.int32)):
                f.write(np.ascontiguousarray(a, dtype=dt).tobytes())
