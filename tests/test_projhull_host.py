"""CPU: the rule of projection_hull_batch (polytope_amd/csrc/plp_projhull.hpp built with g++ -ffp-contract=off,
tests/projhull_host.py), every LP answered by the C oracle's certified LP -- the three checks that define "correct" (outer,
inner, against the reference) on every case of g31, the statuses of the unbounded, flat and overflow cases, the rank step,
the LP budget and the facet cap, and the stand-alone program under the sanitizers."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import projhull_host as PH  # noqa: E402


@pytest.fixture(scope="module")
def LP(tmp_path_factory):
    return PH.build(tmp_path_factory.mktemp("projhull_host"))


@pytest.fixture(scope="module")
def cases():
    return PH.load()


def _run(LP, case, **kw):
    xc = PH.centre(case.A, case.b)
    assert xc is not None
    lp = PH.oracle_lp(case.A, case.b)
    return PH.run(LP, case.A[None], case.b[None], None, case.dim, xc[None], lambda _p, c: lp(c), **kw)


@pytest.fixture(scope="module")
def results(LP, cases):
    """Every case of the fixture through the rule once (shared by the tests below)."""
    return [_run(LP, c) for c in cases]


def test_fixture_is_pinned(cases):
    """At most 2 % of any family may be unpinned (the cap of hull_host.py), and the shapes the issue names are there."""
    fams = sorted({c.family for c in cases})
    assert fams == sorted(["random", "horizon", "box", "triangle", "open", "identity", "line", "overflow"])
    for f in fams:
        mine = [c for c in cases if c.family == f]
        assert sum(not c.pinned for c in mine) <= 0.02 * len(mine), f
    shapes = {(c.A.shape[0] - 2 * c.A.shape[1], c.A.shape[1], len(c.dim)) for c in cases if c.family == "random"}
    assert shapes == {(16, 5, 2), (20, 6, 2), (14, 5, 3), (28, 8, 2)}
    assert sum(c.expect == PH.PH_OVERFLOW_POINTS and c.ref_V.shape[0] > 64 for c in cases) == 2


def test_statuses_and_the_three_checks(cases, results):
    """(a), (b), (c) on every case that has an answer; the expected status everywhere; nlp >= count.  Prints the worst
    excess over ref_gap on the pinned cases: REF_MARGIN (tests/projhull_host.py) is ten times the value measured here."""
    worst_outer, worst_ref = -np.inf, -np.inf
    for c, r in zip(cases, results):
        assert int(r["status"][0]) == c.expect, (c.index, c.family, int(r["status"][0]))
        assert int(r["nlp"][0]) == len(r["asked"]) and int(r["nlp"][0]) >= int(r["m"][0])
        if c.expect != PH.PH_OK:
            assert int(r["m"][0]) == 0 and np.all(np.isnan(r["A"][0])) and np.all(np.isnan(r["b"][0])) and not r["on"][0].any()
            continue
        outer, ref = PH.check_all(c, r, 0)
        worst_outer = max(worst_outer, outer)
        if c.pinned:
            worst_ref = max(worst_ref, ref)
    print("projhull host: worst outer excess %.3g, worst excess over ref_gap %.3g (units of the frame)" % (worst_outer, worst_ref))


def test_unbounded_flat_and_overflow(LP, cases, results):
    by = {c.family: [] for c in cases}
    for c, r in zip(cases, results):
        by[c.family].append((c, r))
    (c_ok, r_ok), (c_unb, r_unb) = by["open"]
    assert int(r_ok["status"][0]) == PH.PH_OK and int(r_unb["status"][0]) == PH.PH_UNBOUNDED
    assert int(r_unb["nlp"][0]) <= 2 * len(c_unb.dim)   # decided inside the box
    for c, r in by["overflow"]:
        assert int(r["status"][0]) == PH.PH_OVERFLOW_POINTS and int(r["nv"][0]) == PH.MAX_POINTS
    # flat: a square in the plane x_3 = 0.25 (an equality as two rows cannot have a strictly interior centre, so the
    # plane is 1e-3 thick in R^3 but the projection onto (x_1, x_3) is asked on a frame that makes it 1e-12 thin)
    A = np.vstack([np.eye(3), -np.eye(3)])
    b = np.array([1.0, 1.0, 0.25 + 1e-12, 1.0, 1.0, -0.25 + 1e-12])
    xc = np.array([0.0, 0.0, 0.25])
    lp = PH.oracle_lp(A, b)
    r = PH.run(LP, A[None], b[None], None, [1, 3], xc[None], lambda _p, c: lp(c))
    assert int(r["status"][0]) == PH.PH_FLAT and int(r["m"][0]) == 0


def test_collinear_start_goes_through_the_rank_step(cases, results):
    (c, r), = [(c, r) for c, r in zip(cases, results) if c.family == "triangle"]
    assert int(r["status"][0]) == PH.PH_OK and int(r["nrank"][0]) == 1 and int(r["m"][0]) == 3 and int(r["nv"][0]) == 3
    got = sorted(map(tuple, np.round(r["V"][0, :3], 12)))
    assert got == [(0.0, 0.0), (0.5, 0.2), (1.0, 1.0)]
    others = [int(r2["nrank"][0]) for c2, r2 in zip(cases, results) if c2.family in ("random", "horizon")]
    assert not any(others)


def test_budget_and_facet_cap(LP, cases):
    c = [c for c in cases if c.family == "random"][0]
    r = _run(LP, c, max_lps=3)
    assert int(r["status"][0]) == PH.PH_BUDGET and int(r["nlp"][0]) == 3 and len(r["asked"]) == 3 and int(r["m"][0]) == 0
    r = _run(LP, c, f_max=2)
    assert int(r["status"][0]) == PH.PH_OVERFLOW_FACETS and int(r["m"][0]) == 0 and r["A"].shape == (1, 2, 2)


def test_no_centre_runs_nothing(LP, cases):
    c = [c for c in cases if c.family == "random"][0]
    lp = PH.oracle_lp(c.A, c.b)
    for xc in (np.full(c.A.shape[1], np.nan), 5.0 * np.ones(c.A.shape[1])):
        r = PH.run(LP, c.A[None], c.b[None], None, c.dim, xc[None], lambda _p, cc: lp(cc))
        assert int(r["status"][0]) == PH.PH_NOCENTRE and not r["asked"] and int(r["nv"][0]) == 0


def test_rows_beyond_m_are_not_read(LP, cases):
    """Two cases of one d packed with NaN beyond m: the same outputs as alone."""
    pair = [c for c in cases if c.family == "random" and c.A.shape[1] == 5 and len(c.dim) == 2][:1] + \
           [c for c in cases if c.family == "open"][:1]
    A, b, m = PH.pack([(c.A, c.b) for c in pair])
    xc = np.array([PH.centre(c.A, c.b) for c in pair])
    lps = [PH.oracle_lp(c.A, c.b) for c in pair]
    r = PH.run(LP, A, b, m, pair[0].dim, xc, lambda p, cc: lps[p](cc))
    for p, c in enumerate(pair):
        alone = _run(LP, c)
        for key in ("A", "b", "on", "m", "V", "nv", "X", "vmask", "nlp", "status"):
            assert np.array_equal(r[key][p], alone[key][0], equal_nan=True), (p, key)


def test_program_under_sanitizers(tmp_path):
    """The same source as a stand-alone program (a cube, a simplex and the collinear triangle with an LP of its own) under
    -fsanitize=address,undefined; nothing is loaded into an interpreter."""
    prog = PH.build_program(tmp_path)
    p = subprocess.run([prog], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "inconsistent: 0" in p.stdout and "runtime error" not in p.stderr
