"""CPU: the candidate rule of the sparse pair calls (polytope_amd/csrc/plp_box_pairs.hpp, compiled for the host by
tests/box_pairs_host.py) -- the sequential grid walk gives exactly the pairs of the brute-force definition, sorted and
without duplicates, with a per_cell that matches; every pair the reference calls adjacent (tests/golden/adjacent_sparse.npz)
is a candidate; plan_pair_list picks the engines plan_pairs picks, sized by K; and the argument errors of the new calls
come back without a device."""
import ctypes as C

import numpy as np
import pytest

import box_pairs_host as H
import polytope_amd as pa
from polytope_amd import _lib

ABS_TOL = 1e-7


@pytest.fixture(scope="module")
def L(tmp_path_factory):
    return H.build(tmp_path_factory.mktemp("box_pairs_host"))


@pytest.fixture(scope="module")
def cases():
    return {c[0]: c[1:] for c in H.box_cases()}


def _check_list(per_cell, pairs, n, n1=0):
    assert per_cell[0] == 0 and per_cell[n] == pairs.shape[0] and np.all(np.diff(per_cell) >= 0)
    # cell i's partners are pairs[per_cell[i] : per_cell[i + 1]]
    assert np.array_equal(pairs[:, 0], np.repeat(np.arange(n), np.diff(per_cell)))
    code = pairs[:, 0].astype(np.int64) * max(n, 1) + pairs[:, 1]
    assert np.all(np.diff(code) > 0), "not sorted by (i, j), or a duplicate"
    if n1:
        assert np.all(pairs[:, 0] < n1) and np.all(pairs[:, 1] >= n1) and np.all(pairs[:, 1] < n)
    else:
        assert np.all(pairs[:, 1] < pairs[:, 0]) and np.all(pairs[:, 1] >= 0)


@pytest.mark.parametrize("name", H.box_case_names())
def test_walk_equals_brute(L, cases, name):
    lb, ub = cases[name]
    n = lb.shape[0]
    for n1 in (0, n // 3):
        per_cell, pairs = H.brute(L, lb, ub, n1)
        _check_list(per_cell, pairs, n, n1)
        lists = H.host_lists(L, lb, ub) if n else None
        if name in ("all_span", "n0", "n1"):
            assert lists is None
        if lists is None:
            continue
        wc, wp = H.walk(L, lb, ub, lists, n1)
        assert np.array_equal(wc, per_cell) and np.array_equal(wp, pairs)


def test_brute_is_the_definition(L, cases):
    """the host's brute force against the rule written out in numpy"""
    pad = pa.batch._LOCATE_PAD
    for name in ("scattered", "halfspace", "empty_nan_inf", "far", "slab"):
        lb, ub = cases[name]
        fin = np.concatenate([np.where(np.isfinite(lb), np.abs(lb), 0), np.where(np.isfinite(ub), np.abs(ub), 0)], 1)
        ps = pad * np.maximum(1.0, fin.max(1))[:, None]
        with np.errstate(invalid="ignore"):
            Lo = np.where(np.isnan(lb), -np.inf, lb)
            Hi = np.where(np.isnan(ub), np.inf, ub)
            Lo = np.where(np.isfinite(Lo), Lo - ps, Lo)
            Hi = np.where(np.isfinite(Hi), Hi + ps, Hi)
        meet = (np.maximum(Lo[:, None], Lo[None]) <= np.minimum(Hi[:, None], Hi[None])).all(-1)
        _, pairs = H.brute(L, lb, ub)
        assert np.array_equal(pairs, H.tril_pairs(meet)), name


def test_slab_and_big_box_counts(L, cases):
    lb, ub = cases["slab"]
    per_cell, pairs = H.brute(L, lb, ub)
    # the slab (cell 0) meets the 12 x 1 strip of cells it crosses plus the rows it touches; each pair once
    assert ((pairs[:, 1] == 0).sum()) >= 12
    lb, ub = cases["big_box"]
    per_cell, pairs = H.brute(L, lb, ub)
    assert per_cell[102] - per_cell[101] == 101 and (pairs[:, 1] == 0).sum() == 101   # more than 64 partners


def test_reference_adjacent_pairs_are_candidates(L):
    """every pair the reference calls adjacent has boxes that meet: outer boxes of the abs_tol-inflated cells"""
    fx = H.load_fixture()
    for name in "abcd":
        f = fx[name]
        A, b, m = f["A"], f["b"], f["m"]
        d = A.shape[2]
        if name == "c":   # (the first 2 d rows of each cell are a cube around it: an outer box)
            lb, ub = H.exact_boxes(A[:, :2 * d], b[:, :2 * d], None, ABS_TOL)
        else:
            lb, ub = H.exact_boxes(A, b, m, ABS_TOL)
        assert np.all(np.isfinite(lb)) and np.all(np.isfinite(ub))
        _, cand = H.brute(L, lb, ub)
        want = H.tril_pairs(f["adj"])
        n = A.shape[0]
        code = set((cand[:, 0].astype(np.int64) * n + cand[:, 1]).tolist())
        missing = [tuple(p) for p in want.tolist() if p[0] * n + p[1] not in code]
        assert not missing, (name, missing[:5])
        assert cand.shape[0] < n * (n - 1) // 2 or name == "d"
    # (a): the 468 touching pairs, corner contacts included, and nothing else is even a candidate
    _, _, idx = H.grid_cells((4, 4, 4))
    assert np.array_equal(H.tril_pairs(fx["a"]["adj"]), H.grid_touching(idx)) and H.grid_touching(idx).shape[0] == 468
    lb, ub = H.exact_boxes(fx["a"]["A"], fx["a"]["b"], None, ABS_TOL)
    assert np.array_equal(H.brute(L, lb, ub)[1], H.grid_touching(idx))


PLAN_CASES = [
    # (n, m_max, d, K, PLP_ADJ_WIDE) -> (engine, gs, workgroups)
    ((257, 10, 6, 4096, None), ("WIDE", 64, 4096)),        # d = 5..8, at most 4096 listed pairs: one pair per wavefront
    ((257, 10, 6, 4097, None), ("GROUP", 8, 513)),         # ... more: lane groups, 8 pairs per workgroup
    ((100000, 10, 6, 4096, None), ("WIDE", 64, 4096)),     # sized by K, not by the n (n - 1) / 2 pairs of the table
    ((257, 17, 6, 100000, None), ("WIDE", 64, 100000)),    # more than 32 stacked rows
    ((257, 10, 9, 100000, None), ("WIDE", 64, 100000)),    # d >= 9 has no lane-group kernel
    ((257, 8, 4, 1000, None), ("GROUP", 4, 63)),           # d <= 4: lane groups, 16 rows on 4 lanes
    ((257, 10, 4, 1000, None), ("GROUP", 8, 125)),
    ((257, 32, 4, 1000, None), ("GROUP", 16, 250)),
    ((257, 10, 6, 100, "0"), ("GROUP", 8, 13)),
    ((257, 10, 5, 100000, "1"), ("WIDE", 64, 100000)),
    ((257, 10, 9, 100, "0"), ("WIDE", 64, 100)),
    ((3, 10, 3, 100, None), ("GROUP", 8, 13)),             # a list may repeat pairs: K beyond n (n - 1) / 2
    ((257, 10, 6, 0, None), ("EMPTY", 0, 0)),
    ((257, 33, 6, 10, None), ("NONE", 0, 0)),
    ((257, 10, 17, 10, None), ("NONE", 0, 0)),
    ((257, 10, 6, -1, None), ("NONE", 0, 0)),
]


@pytest.mark.parametrize("args,want", PLAN_CASES)
def test_plan_pair_list(L, args, want):
    n, m_max, d, K, sw = args
    p = H.plan(L, n, m_max, d, K, sw)
    if want[0] in ("EMPTY", "NONE"):
        assert p["engine"] == want[0]
        return
    assert (p["engine"], p["gs"], p["grid"]) == want and (p["p_lo"], p["p_hi"]) == (0, K)
    assert p["block"] == 64 and p["lds"] == 0


def test_argument_errors_need_no_device():
    lib = _lib.load()
    z = np.zeros(8)
    p = C.c_void_p(z.ctypes.data)
    assert lib.plp_pair_list(None, 2, 4, 2, p, p, None, 0.0, 1e-7, 1, p, p) == _lib.PLP_EINVAL
    assert b"ctx is NULL" in lib.plp_last_error()
    assert lib.plp_pair_list_dev(None, None, 2, 4, 2, p, p, None, 0.0, 1e-7, 1, p, p) == _lib.PLP_EINVAL
    assert lib.plp_box_pairs_count(None, 2, 2, p, p, 0.0, None, None, None, 0, p) == _lib.PLP_EINVAL
    assert lib.plp_box_pairs_count_dev(None, None, 2, 2, p, p, 0.0, None, None, None, 0, p) == _lib.PLP_EINVAL
    assert lib.plp_box_pairs_fill(None, 2, 2, p, p, 0.0, None, None, None, 0, p, 0, 2, p) == _lib.PLP_EINVAL
    assert lib.plp_box_pairs_fill_dev(None, None, 2, 2, p, p, 0.0, None, None, None, 0, p, 0, 2, p) == _lib.PLP_EINVAL
    A, b = np.zeros((3, 4, 2)), np.zeros((3, 4))
    with pytest.raises(ValueError):
        pa.pair_verdicts(A, b, np.zeros((5, 3), np.int32))
    with pytest.raises(ValueError):
        pa.box_pairs(np.zeros((3, 2)), np.zeros((4, 2)))
    with pytest.raises(ValueError):
        pa.box_pairs(np.zeros((3, 2)), np.zeros((3, 2)), grid="dense")
    with pytest.raises(ValueError):
        pa.box_pairs(np.zeros((3, 2)), np.zeros((3, 2)), n1=4)
    with pytest.raises(_lib.UnsupportedSize):
        pa.box_pairs(np.zeros((3, 17)), np.zeros((3, 17)))
    with pytest.raises(_lib.UnsupportedSize):
        pa.adjacent_pairs_sparse(np.zeros((3, 33, 2)), np.zeros((3, 33)))
    with pytest.raises(_lib.UnsupportedSize):
        pa.overlap_pairs_sparse(np.zeros((3, 4, 17)), np.zeros((3, 4)))
    with pytest.raises(ValueError):
        pa.adjacent_pairs_sparse(A, b, max_candidates=0)
    with pytest.raises(ValueError):
        pa.adjacent_pairs_sparse(A, b, boxes=(np.zeros((2, 2)), np.zeros((2, 2))))
    with pytest.raises(ValueError):
        pa.adjacent_pairs_sparse(np.full((3, 4, 2), np.inf), b)
