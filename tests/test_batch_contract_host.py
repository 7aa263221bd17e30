"""CPU: the packed-table contract of include/plp.h on the host builds of the rule headers (tests/cabi/hull_enum_host.cpp,
extreme_host.cpp, support_host.cpp, volume_host.cpp, fm_host.cpp): rows from m[p] on, points from n[p] on and rows or points
whose keep bit is clear do not exist -- whatever they hold (NaN, 1e300, values that would change the answer), every output
bit is the one the zero-padded call gives.  And an outside reference for the two enumeration rules: the facets of lattice
point sets and the vertices of integer-row polytopes in exact rational arithmetic (tests/contract_cases.py), on inputs
whose smallest non-zero distance keeps a factor 1000 clear of the rules' tolerances, so that the exact rule and the
tolerant one cannot disagree.  tests/test_batch_contract_gpu.py holds the device to the same."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import contract_cases as cc  # noqa: E402
import extreme_host as xh  # noqa: E402
import fm_host as fh  # noqa: E402
import hull_host as hh  # noqa: E402
import support_host as sh  # noqa: E402
import volume_host as vh  # noqa: E402

POISONS = ("nan", "huge", "cut")
ENUM_SHAPES = [(5, 2), (16, 3), (12, 4), (64, 2)]


@pytest.fixture(scope="module")
def HL(tmp_path_factory):
    return hh.build(tmp_path_factory.mktemp("hull_host"))


@pytest.fixture(scope="module")
def XL(tmp_path_factory):
    return xh.build(tmp_path_factory.mktemp("extreme_host"))


@pytest.fixture(scope="module")
def SL(tmp_path_factory):
    return sh.build(tmp_path_factory.mktemp("support_host"))


@pytest.fixture(scope="module")
def VL(tmp_path_factory):
    return vh.build(tmp_path_factory.mktemp("volume_host"))


@pytest.fixture(scope="module")
def FL(tmp_path_factory):
    return fh.build(tmp_path_factory.mktemp("fm_host"))


def assert_same(got, want, what):
    """Two tuples / dicts of arrays, every one bit for bit (int64 views: NaN compares as its bits)."""
    if isinstance(want, dict):
        keys = sorted(k for k in want if want[k] is not None)
        got, want = [got[k] for k in keys], [want[k] for k in keys]
    else:
        keys = list(range(len(want)))
    for k, g, w in zip(keys, got, want):
        assert cc.same_bits(g, w), (what, k, np.argwhere(np.asarray(g) != np.asarray(w))[:4].tolist())


# ------------------------------------------------------------------------------------------------ the poison itself
def test_poison_touches_the_padding_only_and_cut_would_change_the_answer(XL, HL):
    """poison() leaves every live slot as it was and overwrites every other one; and its "cut" values, read as live rows
    or points (m = m_max, no keep word), do change the answer of every member that has padding: the finite poison is one a
    kernel that read it would not get away with."""
    A, b, m = cc.mixed_rows(9, 12, 3, seed=1)
    keep = cc.keep_words(np.random.default_rng(2), 9, forced=6)
    dead = cc._dead(m, 12, keep)
    for kind in cc.KINDS:
        Ap, bp = cc.poison((A, b), m, kind, keep)
        assert np.array_equal(Ap[~dead], A[~dead]) and np.array_equal(bp[~dead], b[~dead])
        if kind == "nan":
            assert np.all(np.isnan(Ap[dead])) and np.all(np.isnan(bp[dead]))
        if kind == "huge":
            assert np.all(Ap[dead] == cc.HUGE) and np.all(bp[dead] == cc.HUGE)
    assert dead[0].sum() == 0 and dead[1].all() and dead[2:].any(axis=1).all()
    v_max = xh.vmax_for(3, 12)
    Ap, bp = cc.poison((A, b), m, "cut")
    base = xh.run(XL, A, b, m, None, v_max)
    read = xh.run(XL, Ap, bp, None, None, v_max)
    for p in np.nonzero(m < 12)[0]:
        if base[3][p] == xh.XS_EMPTY:   # (no rows, the empty member: nothing left to take away for this rule)
            assert p in (1, 3)
            continue
        assert not (cc.same_bits(read[0][p], base[0][p]) and read[3][p] == base[3][p]), p
        assert read[3][p] == xh.XS_EMPTY or p == 2, p   # (member 2 is a cone: cut, not emptied)
    X, n = cc.mixed_points(9, 12, 3, seed=3)
    Xp, = cc.poison((X,), n, "cut", what="points")
    base = hh.run(HL, X, n)
    read = hh.run(HL, Xp, None)
    for p in np.nonzero(n < 12)[0]:
        assert not cc.same_bits(read["on"][p], base["on"][p]) or read["status"][p] != base["status"][p], p


# ------------------------------------------------------------------------------------------------ padding is not read
@pytest.mark.parametrize("n_max,d", ENUM_SHAPES)
def test_hull_host_reads_no_padding(HL, n_max, d):
    """Ragged n from 0 to n_max, keep words with holes, with and without `basis`."""
    B = 9
    X, n = cc.mixed_points(B, n_max, d, seed=100 * d + n_max)
    keep = cc.keep_words(np.random.default_rng(n_max), B, forced=d + 1)
    assert n[0] == n_max and n[1] == 0 and n.min() == 0
    for kp in (None, keep):
        want = hh.run(HL, *cc.poison((X,), n, "zero", kp, what="points"), n, kp)
        assert (want["status"] == hh.HS_OK).any() and (want["status"] == hh.HS_FLAT).any()
        for kind in POISONS:
            Xp, = cc.poison((X,), n, kind, kp, what="points")
            assert_same(hh.run(HL, Xp, n, kp), want, ("hull", kind, kp is not None))


@pytest.mark.parametrize("m_max,d", ENUM_SHAPES)
def test_extreme_host_reads_no_padding(XL, m_max, d):
    """Ragged m from 0 to m_max, keep words with holes (a hole in the box leaves an unbounded member: it has the vertices
    the rule finds)."""
    B = 9
    A, b, m = cc.mixed_rows(B, m_max, d, seed=200 * d + m_max)
    keep = cc.keep_words(np.random.default_rng(m_max), B, forced=d)
    assert m[0] == m_max and m[1] == 0
    v_max = xh.vmax_for(d, m_max)
    for kp in (None, keep):
        want = xh.run(XL, *cc.poison((A, b), m, "zero", kp), m, kp, v_max)
        assert (want[3] == xh.XS_OK).any() and (want[3] == xh.XS_EMPTY).any()
        for kind in POISONS:
            Ap, bp = cc.poison((A, b), m, kind, kp)
            assert_same(xh.run(XL, Ap, bp, m, kp, v_max), want, ("extreme", kind, kp is not None))


@pytest.mark.parametrize("shared", [True, False], ids=["shared", "own"])
@pytest.mark.parametrize("m_max,d", [(7, 2), (16, 3), (20, 4)])
def test_support_host_reads_no_padding(SL, m_max, d, shared):
    """K = 5 directions, shared or per polytope, from the origin (strictly inside every member that has an inside; the
    empty and the flat member are handed back, status 1, under every poison alike)."""
    B, K = 9, 5
    A, b, m = cc.mixed_rows(B, m_max, d, seed=300 * d + m_max)
    rng = np.random.default_rng(m_max + 7)
    C_ = rng.standard_normal((K, d) if shared else (B, K, d))
    xc = np.zeros((B, d))
    want = sh.run(SL, A, b, C_, xc, m)
    assert (want[2] == 0).any() and (want[2] == 3).any() and (want[2] == 1).any()
    for kind in POISONS:
        Ap, bp = cc.poison((A, b), m, kind)
        assert_same(sh.run(SL, Ap, bp, C_, xc, m), want, ("support", kind))


@pytest.mark.parametrize("d", [1, 3, 4])
def test_volume_host_reads_no_padding(VL, d):
    """N = 777 samples per member in the box [-3.1, 3.1]^d; m = 0 is VF_NOROWS."""
    B, m_max, N = 9, 2 * d + 5, 777
    A, b, m = cc.mixed_rows(B, m_max, d, seed=400 + d)
    lb, ub = np.full((B, d), -3.1), np.full((B, d), 3.1)
    words = [vh.seed_state(1000 + p) for p in range(B)]
    state, inc = np.array([w[0] for w in words]), np.array([w[1] for w in words])
    want = vh.hits(VL, A, b, lb, ub, state, inc, N, m=m)
    assert want[1][1] == 2 and not want[1][[0, 2, 5]].any() and 0 < want[0][0] < N
    for kind in POISONS:
        Ap, bp = cc.poison((A, b), m, kind)
        assert_same(vh.hits(VL, Ap, bp, lb, ub, state, inc, N, m=m), want, ("volume", kind))


@pytest.mark.parametrize("first", [False, True], ids=["later", "first"])
@pytest.mark.parametrize("m_max,d", [(10, 3), (14, 4)])
def test_fm_host_reads_no_padding(FL, m_max, d, first):
    """One elimination step on the last column and the step without elimination (col < 0), with m alone, with a keep word
    with holes, and with keep and flags (a minimal representation, an empty one)."""
    B = 9
    A, b, m = cc.mixed_rows(B, m_max, d, seed=500 * d + m_max)
    keep = cc.keep_words(np.random.default_rng(m_max + 1), B, forced=2)
    flags = np.array([0, 0, 4, 1, 4, 0, 4, 2, 0], np.int32)
    for col in (d - 1, -1):
        for kp, fl in ((None, None), (keep, None), (keep, flags)):
            want = fh.step(FL, *cc.poison((A, b), m, "zero", kp), col, m=m, keep=kp, flags=fl, first=first)
            assert want[0].max() > 0 and want[0][1] == 0 and (want[3] >= 0).all()
            for kind in POISONS:
                Ap, bp = cc.poison((A, b), m, kind, kp)
                got = fh.step(FL, Ap, bp, col, m=m, keep=kp, flags=fl, first=first, mo_max=want[1].shape[1])
                assert_same(got, want, ("fm", kind, col, kp is not None, fl is not None))


# ------------------------------------------------------------------------------------------------ exact references
@pytest.mark.parametrize("d", [2, 3, 4])
def test_hull_host_equals_the_exact_hull(HL, d):
    """contract_cases.HULL_CASES lattice sets per dimension (flat ones, exact repeats and a set of too few points among them), packed
    with answer-changing padding: status, count and the incidence sets are the exact hull's, every row a unit normal that
    holds its incident points to 1e-9 of the extent.  No case is left out: each keeps MIN_DISTANCE clear."""
    sets = cc.lattice_sets(d, cc.HULL_CASES[d], seed=70 + d)
    X, n = cc.pack_points(sets)
    Xp, = cc.poison((X,), n, "cut", what="points")
    res = hh.run(HL, Xp, n)
    seen = set()
    for k, pts in enumerate(sets):
        least = cc.check_hull(pts, res["A"][k], res["b"][k], res["on"][k], int(res["count"][k]), int(res["status"][k]))
        assert least >= cc.MIN_DISTANCE, (d, k, least)
        seen.add(int(res["status"][k]))
    assert seen == {hh.HS_OK, hh.HS_FLAT}


@pytest.mark.parametrize("d", [2, 3, 4])
def test_extreme_host_equals_the_exact_vertices(XL, d):
    """contract_cases.VERTEX_CASES integer-row polytopes per dimension (a repeated row, a flat polytope and two empty ones among them),
    packed with answer-changing padding: status and count are the exact ones, the vertices agree both ways to
    extreme_host.MATCH max(1, |v|).  No case is left out: each keeps MIN_DISTANCE clear."""
    cases = cc.integer_polytopes(d, cc.VERTEX_CASES[d], seed=80 + d)
    A, b, m = cc.pack_rows(cases)
    Ap, bp = cc.poison((A, b), m, "cut")
    V, count, _, status = xh.run(XL, Ap, bp, m, None, xh.vmax_for(d, A.shape[1]))
    seen = set()
    for k, (Ak, bk) in enumerate(cases):
        least = cc.check_vertices(Ak, bk, V[k], int(count[k]), int(status[k]), xh.MATCH)
        assert least >= cc.MIN_DISTANCE, (d, k, least)
        seen.add(int(status[k]))
    assert seen == {xh.XS_OK, xh.XS_EMPTY}
