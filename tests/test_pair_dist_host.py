"""CPU: the per-pair function of pair_dist_kernel (polytope_amd/csrc/plp_pair_dist.hpp) in its host build
(tests/cabi/pair_dist_host.cpp), held against two independent references (tests/pair_dist_host.py):

 (a) axis boxes in d = 1 .. 4 on a 3^d grid with gaps, every ordered pair, against the closed form
     dist = | max(0, lo_j - hi_i, lo_i - hi_j) |: face-, edge- and corner-touching pairs (dist = 0), nested and equal boxes;
 (b) a duality proof per status-0 answer with the oracle's LPs: x and y feasible to 1e-9 E, dist = |x - y|, and for
     dist > 1e-9 E the oracle's  min over cell i of u.x' - max over cell j of u.y',  u = (x - y) / dist, reaches dist - 1e-9 E
     (weak duality then proves optimality), with lb within 1e-9 E of that value and not above dist.

Tables: every soak family at SOAK_SHAPES, 30 cells each translated by a random offset of 0 .. 4 extents (separated, touching
and overlapping pairs all occur), 200 listed pairs per table with repeats and both orders.  Raw status 1 is allowed up to
a cap, counted per family over the pairs whose two cells are bounded with an oracle Chebyshev radius above 1e-6 of the
extent: 0.02 on random, ragged, scaled and lattice, 0.20 on dup and flat; `unbounded` is counted apart (status 3 may occur
there).  Measured shares (this file's tables): random 0, ragged 0, scaled 0, lattice 0, flat 0, dup 0.057, unbounded 0.001.
Then cases by hand, the symmetry of (i, j) and (j, i), and the stand-alone program under the sanitizers."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import pair_dist_host as ph  # noqa: E402


@pytest.fixture(scope="module")
def L(tmp_path_factory):
    return ph.build(tmp_path_factory.mktemp("pair_dist_host"))


@pytest.mark.parametrize("d", [1, 2, 3, 4])
def test_axis_boxes_equal_the_closed_form(L, d):
    """(a): every ordered pair of the grid's boxes, the box that holds eight of them, the nested one and the copy."""
    lo, hi = ph.box_grid(d)
    A, b, xc = ph.boxes_as_cells(lo, hi)
    P = ph.all_pairs(lo.shape[0])
    out = ph.run(L, A, b, xc, P)
    ref = ph.box_distance(lo, hi, P)
    assert (ref == 0).sum() >= 8 * d and (ref > 0).sum() >= 8 * d   # (touching / nested / equal pairs, and gaps)
    st = out["status"]
    assert set(np.unique(st).tolist()) <= {0, 1}
    assert (st == 1).sum() <= 0.02 * st.size, (st == 1).sum()
    ok = st == 0
    E = np.maximum(1.0, np.maximum(np.abs(out["x"]).max(axis=1), np.abs(out["y"]).max(axis=1)))
    assert np.all(np.abs(out["dist"] - ref)[ok] <= ph.TOL * E[ok]), np.nanmax(np.abs(out["dist"] - ref))
    assert np.all(out["x"][ok] >= lo[P[ok, 0]] - ph.TOL * E[ok, None]) and np.all(out["x"][ok] <= hi[P[ok, 0]] + ph.TOL * E[ok, None])
    assert np.all(out["y"][ok] >= lo[P[ok, 1]] - ph.TOL * E[ok, None]) and np.all(out["y"][ok] <= hi[P[ok, 1]] + ph.TOL * E[ok, None])
    assert np.all(np.abs(np.linalg.norm(out["x"] - out["y"], axis=1) - out["dist"])[ok] <= 1e-12 * E[ok])
    assert np.all(out["lb"][ok] <= out["dist"][ok]) and np.all(out["lb"][ok] >= out["dist"][ok] - ph.TOL * E[ok])
    assert np.all(out["rounds"] <= L.pair_dist_max_rounds())


@pytest.mark.parametrize("fam", ph.FAMILIES)
def test_soak_families_pass_the_duality_proof(L, oracle, fam):
    """(b) on every status-0 answer of the family's six tables, the statuses, and the hand-back cap."""
    counted = back = checked = 0
    for T in ph.tables(oracle, fam):
        out = ph.run(L, T["A"], T["b"], T["xc"], T["pairs"], T["m"])
        ph.check_statuses(T, out)
        checked += ph.check_duality(oracle, T, out)
        c = ph.counted(T)
        counted += int(c.sum())
        back += int((out["status"][c] == 1).sum())
        no_centre = ~np.isfinite(T["xc"]).all(axis=1)
        assert np.all(out["status"][no_centre[T["pairs"][:, 0]] | no_centre[T["pairs"][:, 1]]] == 1)
        bare = ph.run(L, T["A"], T["b"], T["xc"], T["pairs"], T["m"], points=False)
        assert ph.hb.same_bits(bare["dist"], out["dist"]) and np.array_equal(bare["status"], out["status"])
    print("%s: %d counted pairs, %d handed back (%.4f), %d answers proved" % (fam, counted, back, back / max(1, counted), checked))
    assert counted > 0 and checked > 0
    if fam in ph.HANDBACK_CAPS:
        assert back <= ph.HANDBACK_CAPS[fam] * counted, (fam, back, counted)


@pytest.mark.parametrize("fam", ["random", "dup"])
def test_both_orders_agree(L, oracle, fam):
    """(i, j) and (j, i): the same distance to 1e-9 E, x and y swapped (where both orders settle)."""
    n = 0
    for T in ph.tables(oracle, fam):
        P = T["pairs"]
        a = ph.run(L, T["A"], T["b"], T["xc"], P, T["m"])
        r = ph.run(L, T["A"], T["b"], T["xc"], P[:, ::-1], T["m"])
        both = (a["status"] == 0) & (r["status"] == 0)
        E = np.maximum(1.0, np.maximum(np.abs(a["x"]).max(axis=1), np.abs(a["y"]).max(axis=1)))
        assert np.all(np.abs(a["dist"] - r["dist"])[both] <= ph.TOL * E[both])
        # x and y swapped: the second call's y lies in cell i and its x in cell j (the closest points need not be unique)
        for t in np.nonzero(both)[0]:
            i, j = P[t]
            for cell, pt in ((i, r["y"][t]), (j, r["x"][t])):
                Ac, bc = T["A"][cell, :T["m"][cell]], T["b"][cell, :T["m"][cell]]
                nrm = np.linalg.norm(Ac, axis=1)
                assert np.max((Ac @ pt - bc) / np.where(nrm > 0, nrm, 1.0), initial=-np.inf) <= ph.TOL * E[t], (t, cell)
        n += int(both.sum())
    assert n > 500


def hand_table():
    """Six cells at (8, 3): the unit box, the same moved by (3, 0, 0), an empty set, a single point, m = 0, a box whose centre
    is given as NaN."""
    d = 3
    box = np.vstack([np.eye(d), -np.eye(d)])
    A, b = np.zeros((6, 8, d)), np.zeros((6, 8))
    A[:, :6], b[:, :6] = box, 1.0
    b[1, :6] = [4.0, 1.0, 1.0, -2.0, 1.0, 1.0]
    A[2, 6], b[2, 6] = [1.0, 1.0, 0.0], -3.0             # empty: x + y <= -3 inside the unit box
    b[3, :6] = [2.5, 0.25, 0.0, -2.5, -0.25, 0.0]        # the single point (2.5, 0.25, 0)
    m = np.array([6, 6, 7, 6, 0, 6], np.int32)
    xc = np.zeros((6, d))
    xc[1] = [3.0, 0.0, 0.0]
    xc[2] = np.nan                                       # (no interior point: what cheby_ball_batch gives it)
    xc[3] = [2.5, 0.25, 0.0]                             # on the boundary of all six rows: not strictly inside
    xc[5] = np.nan
    return A, b, m, xc


def test_cases_by_hand(L):
    A, b, m, xc = hand_table()
    P = np.array([[0, 1], [1, 0], [0, 2], [0, 3], [0, 4], [4, 1], [0, 5], [5, 1]], np.int32)
    out = ph.run(L, A, b, xc, P, m)
    assert out["status"].tolist() == [0, 0, 1, 1, 3, 3, 1, 1]
    assert np.allclose(out["dist"][:2], 1.0, rtol=0, atol=1e-12) and np.allclose(out["lb"][:2], 1.0, rtol=0, atol=1e-9)
    assert np.allclose(out["x"][0, 0], 1.0, atol=1e-12) and np.allclose(out["y"][0, 0], 2.0, atol=1e-12)
    assert np.allclose(out["x"][1, 0], 2.0, atol=1e-12) and np.allclose(out["y"][1, 0], 1.0, atol=1e-12)
    assert np.all(np.isnan(out["dist"][2:])) and np.all(np.isnan(out["x"][2:])) and np.all(np.isnan(out["lb"][2:]))
    # the host-pointer contract: a pair (i, i) or an index outside [0, n) is refused before anything runs
    for bad in ([[0, 1], [2, 2]], [[0, 6]], [[-1, 0]]):
        ph.run(L, A, b, xc, np.array(bad, np.int32), m, expect=1)
    # no pairs: nothing to do
    assert ph.run(L, A, b, xc, np.zeros((0, 2), np.int32), m)["dist"].shape == (0,)


def test_rows_beyond_m_are_not_read(L, oracle):
    """Poisoned rows beyond m[p] change no output bit."""
    T = ph.tables(oracle, "ragged")[2]
    out = ph.run(L, T["A"], T["b"], T["xc"], T["pairs"], T["m"])
    A, b = T["A"].copy(), T["b"].copy()
    dead = np.arange(A.shape[1])[None, :] >= T["m"][:, None]
    A[dead], b[dead] = np.nan, np.nan
    got = ph.run(L, A, b, T["xc"], T["pairs"], T["m"])
    for k in ph.KEYS:
        assert ph.hb.same_bits(got[k], out[k]) if got[k].dtype == np.float64 else np.array_equal(got[k], out[k]), k


def test_program_under_the_sanitizers(tmp_path, oracle):
    """The stand-alone program (-fsanitize=address,undefined, its own main) on the recorded tables of every family, the box
    grid and the hand cases, and on the cells it makes itself."""
    exe = ph.build_program(tmp_path)
    recs = []
    for fam in ph.FAMILIES:
        for T in ph.tables(oracle, fam):
            recs.append((T["A"], T["b"], T["m"], T["xc"], T["pairs"]))
    lo, hi = ph.box_grid(3)
    A, b, xc = ph.boxes_as_cells(lo, hi)
    recs.append((A, b, None, xc, ph.all_pairs(lo.shape[0])))
    A, b, m, xc = hand_table()
    recs.append((A, b, m, xc, ph.all_pairs(6)))
    path = str(tmp_path / "records.bin")
    ph.write_records(path, recs)
    for args in ([path], []):
        r = ph.run_program(exe, args)
        assert r.returncode == 0, r.stdout[-2000:]
        assert "inconsistent: 0" in r.stdout
