"""The cap sweeps of tests/test_{extreme,hull}_{host,gpu}.py: members whose candidates take two rounds of 64 in the kernel, so
that the overflow (a distinct candidate arriving at count == cap) is reached in a LATER round than the first accepted entry --
the regular 12-gon, C(12, 2) = 66 candidates with the last entry from subset (10, 11) of rank 65, and one random (9, 3)
member, C(9, 3) = 84 candidates -- and the check that every cap gives the first entries of the full list."""
from math import comb

import numpy as np

import extreme_host as xh
import hull_host as hh
from host_build import same_bits, upper_bound


def subset_rank(idx, n):
    """The lexicographic rank of the increasing subset idx among the len(idx)-subsets of range(n)."""
    r, prev = 0, -1
    for k, c in enumerate(idx):
        r += sum(comb(n - 1 - j, len(idx) - 1 - k) for j in range(prev + 1, c))
        prev = c
    return r


def gon12():
    """The corners of the regular 12-gon on the unit circle [12, 2]: the rows x.p_k <= 1, or the points."""
    t = 2.0 * np.pi * np.arange(12) / 12.0
    return np.stack([np.cos(t), np.sin(t)], axis=1)


def extreme_members():
    """[(A[m, d], b[m])]: the 12-gon as rows, one random bounded (9, 3) polytope."""
    from polytope_amd.synth import random_hpolytopes
    A, b = random_hpolytopes(1, 9, 3, seed=11, bounded=True)
    return [(gon12(), np.ones(12)), (A[0], b[0])]


def hull_members():
    """[X[n, d]]: the 12-gon as points, nine random points in d = 3."""
    return [gon12(), np.random.default_rng(11).standard_normal((9, 3))]


def check_extreme(A, b, run_at):
    """run_at(A[1, m, d], b[1, m], v_max) -> (V, count, basis, status).  For every cap k from 1 to the full count + 1 the
    result is the first k entries of the full list bit for bit, basis included, OVERFLOW exactly when k < the full count,
    NaN / -1 beyond the count.  -> (V, count, basis) of the full list."""
    V, count, basis, status = run_at(A[None], b[None], upper_bound(A.shape[1], A.shape[0]) + 1)
    full = int(count[0])
    assert status[0] == xh.XS_OK and full >= 2
    for k in range(1, full + 2):
        Vk, ck, bk, sk = run_at(A[None], b[None], k)
        c = min(k, full)
        assert ck[0] == c and sk[0] == (xh.XS_OVERFLOW if k < full else xh.XS_OK), (k, ck, sk)
        assert same_bits(Vk[0, :c], V[0, :c]) and np.array_equal(bk[0, :c], basis[0, :c]), k
        assert np.all(np.isnan(Vk[0, c:])) and np.all(bk[0, c:] == -1), k
    return V[0], full, basis[0]


def check_hull(X, run_at):
    """run_at(X[1, n, d], f_max) -> a result dict.  As check_extreme, `on` and basis included; NaN / 0 / -1 beyond the
    count.  -> (the full result, its count)."""
    whole = run_at(X[None], upper_bound(X.shape[1], X.shape[0]) + 1)
    full = int(whole["count"][0])
    assert whole["status"][0] == hh.HS_OK and full >= 2
    for k in range(1, full + 2):
        r = run_at(X[None], k)
        c = min(k, full)
        assert r["count"][0] == c and r["status"][0] == (hh.HS_OVERFLOW if k < full else hh.HS_OK), (k, r["count"], r["status"])
        assert same_bits(r["A"][0, :c], whole["A"][0, :c]) and same_bits(r["b"][0, :c], whole["b"][0, :c]), k
        assert np.array_equal(r["on"][0, :c], whole["on"][0, :c]) and np.array_equal(r["basis"][0, :c], whole["basis"][0, :c]), k
        assert np.all(np.isnan(r["A"][0, c:])) and np.all(np.isnan(r["b"][0, c:])), k
        assert np.all(r["on"][0, c:] == 0) and np.all(r["basis"][0, c:] == -1), k
    return whole, full
