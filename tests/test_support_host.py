"""CPU: the per-LP function of support_kernel (polytope_amd/csrc/plp_support.hpp: rows staged as a_i / beta_i, the lane
walk, the end check, the status mapping) compiled for the HOST (tests/cabi/support_host.cpp) and held against the oracle's
simplex, and the argument checks of batch.support_batch that need no library.

Tolerance (tests/support_host.py: check_against_oracle): status equal to oracle.lp_solve's; where it is 0,
|h - (-fun)| <= 1e-9 max(1, |h|); x is not compared (ties have no unique vertex) but A x <= b + 1e-9 and
|c.x - h| <= 1e-12 max(1, |h|)."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import support_host as sh  # noqa: E402


@pytest.fixture(scope="module")
def L(tmp_path_factory):
    return sh.build(tmp_path_factory.mktemp("support_host"))


def family_case(O, k, shared):
    """Family k with its directions, oracle centres and oracle answers (computed once per session)."""
    def make():
        A, b, m = sh.family(k)
        C_ = sh.directions(k, A.shape[0], shared)
        xc = sh.centres(O, A, b, m)
        ost, oh = sh.oracle_support(O, A, b, m, C_)
        return A, b, m, C_, xc, ost, oh
    return sh.memo(("family", k, shared), make)


@pytest.mark.parametrize("shared", [True, False])
@pytest.mark.parametrize("k", range(len(sh.SHAPES)))
def test_random_families_equal_the_oracle(L, oracle, k, shared):
    """B = 40 ragged polytopes per (m, d), 9 random directions plus +-e_i, both layouts of C, centre from oracle.cheby."""
    A, b, m, C_, xc, ost, oh = family_case(oracle, k, shared)
    h, x, st = sh.run(L, A, b, C_, xc, m)
    assert set(np.unique(st)) <= {0, 1, 3}
    sh.check_against_oracle(A, b, m, C_, h, x, st, ost, oh, where=(st != 1))
    assert np.all(np.isnan(h[st == 1])) and np.all(np.isnan(x[st == 1]))
    # without points: the same values, bit for bit
    h2, x2, st2 = sh.run(L, A, b, C_, xc, m, points=False)
    assert x2 is None and np.array_equal(st, st2) and np.array_equal(h, h2, equal_nan=True)


def test_handback_cap_on_the_random_family(L, oracle):
    """Raw status 1 over all the random bounded families: at most 1 % of the LPs."""
    n = back = 0
    for k in range(len(sh.SHAPES)):
        for shared in (True, False):
            A, b, m, C_, xc, _, _ = family_case(oracle, k, shared)
            st = sh.run(L, A, b, C_, xc, m)[2]
            n += st.size
            back += int((st == 1).sum())
    assert n >= 7000 and back <= sh.HANDBACK_CAP * n, (back, n)


@pytest.mark.parametrize("k", range(len(sh.SHAPES)))
def test_unbounded_polytopes(L, oracle, k):
    """random_hpolytopes(bounded=False), ragged: a direction inside the recession cone's dual gives 3, the others 0 -- the
    oracle's verdicts.  The origin is strictly inside every polytope of the generator."""
    A, b, m = sh.family(k, bounded=False)
    C_ = sh.directions(k, A.shape[0], True)
    ost, oh = sh.oracle_support(oracle, A, b, m, C_)
    h, x, st = sh.run(L, A, b, C_, np.zeros((A.shape[0], A.shape[2])), m)
    sh.check_against_oracle(A, b, m, C_, h, x, st, ost, oh, where=(st != 1))
    assert (st == 3).sum() > 20 and (st == 0).sum() > 20 and (st == 1).sum() <= sh.HANDBACK_CAP * st.size
    assert np.all(h[st == 3] == np.inf) and np.all(np.isnan(x[st == 3]))


def test_centre_on_a_facet_or_not_a_point_is_handed_back(L):
    """xc on a facet (beta = 0 on a live row), outside, or NaN: every direction of that polytope comes back as status 1;
    the neighbour with a proper centre is solved."""
    d = 3
    box = np.vstack([np.eye(d), -np.eye(d)])
    A = np.broadcast_to(box, (4, 6, d)).copy()
    b = np.full((4, 6), 2.0)
    xc = np.array([[2.0, 0.0, 0.0], [0.5, 0.25, 0.0], [3.0, 0.0, 0.0], [np.nan, 0.0, 0.0]])
    C_ = np.vstack([np.eye(d), -np.eye(d), np.ones((1, d)), np.zeros((1, d))])
    h, x, st = sh.run(L, A, b, C_, xc)
    assert np.all(st[[0, 2, 3]] == 1) and np.all(np.isnan(h[[0, 2, 3]]))
    assert np.all(st[1] == 0) and np.allclose(h[1], [2, 2, 2, 2, 2, 2, 6, 0], rtol=0, atol=1e-12)
    assert np.array_equal(x[1, 7], xc[1])   # the zero direction: the centre itself
    # a dead row (i >= m) the centre violates does not count
    m = np.array([6, 5, 6, 6], np.int32)
    A[1, 5] = [1.0, 0.0, 0.0]
    b[1, 5] = -7.0
    st2 = sh.run(L, A, b, C_[[0, 1, 5]], xc, m)[2]   # e_0, e_1, -e_2: nothing bounds x_2 from below any more
    assert np.all(st2[1] == [0, 0, 3])


def test_tile_table(L):
    """Polytopes per workgroup: 64 / (lanes for K directions), capped at 64 / 32 / 16 for 16 / 32 / 64 row slots."""
    got = {(K, mm): L.support_polytopes_per_group(K, mm) for K in (1, 2, 3, 6, 32, 33, 64, 65, 130) for mm in (16, 17, 33, 64)}
    for mm, cap in ((16, 64), (17, 32), (33, 16), (64, 16)):
        assert [got[K, mm] for K in (1, 2, 3, 6, 32, 33, 64, 65, 130)] == [min(v, cap) for v in (64, 32, 16, 8, 2, 1, 1, 1, 1)]
    assert L.support_polytopes_per_group(4, 65) == 0


def test_argument_errors_need_no_library(monkeypatch):
    """Wrong rank of C, d mismatch, B mismatch, K = 0, a bad xc: ValueError before anything of the library is touched."""
    from polytope_amd import _lib, batch

    def no_library(*a, **kw):
        raise AssertionError("the library was touched")
    monkeypatch.setattr(_lib, "load", no_library)
    monkeypatch.setattr(_lib, "context", no_library)
    A, b = np.zeros((3, 6, 2)), np.ones((3, 6))
    for C_ in (np.zeros(2), np.zeros((2, 3, 4, 2)), np.zeros((4, 3)), np.zeros((3, 4, 3)), np.zeros((2, 4, 2)),
               np.zeros((0, 2)), np.zeros((3, 0, 2))):
        with pytest.raises(ValueError):
            batch.support_batch(A, b, C_)
    with pytest.raises(ValueError):
        batch.support_batch(A, b, np.zeros((4, 2)), xc=np.zeros((2, 2)))
    with pytest.raises(ValueError):
        batch.support_batch(np.zeros((6, 2)), np.ones(6), np.zeros((4, 2)))
    with pytest.raises(ValueError):
        batch.subset_batch(A, b, np.zeros((6, 2)), np.ones(6))
