"""CPU: the per-problem function of nearest_kernel (polytope_amd/csrc/plp_nearest.hpp: rows staged at unit norm, the dual
active-set walk, the two end checks, the Farkas check, the status mapping) compiled for the HOST
(tests/cabi/nearest_host.cpp) and held against references written out in tests/nearest_host.py, and the argument checks
of batch.nearest_batch that need no library.

Every raw status-0 answer, with E = max(1, |x|_inf, |p|_inf):
    feasibility           max_i (n_i.x - beta_i) <= 1e-9 E
    dist                  equal to |x - p|_2 to 1e-12 relative
    against the reference |dist - dist_ref| <= 1e-9 E  (the project's LP tolerance, support_host.check_against_oracle; by the
                          projection inequality |x - x_ref|^2 <= 2 dist 1e-9 E + the feasibility slack)
    well-separated rows   also |x - x_ref|_inf <= 1e-9 E
    the certificate       the kernel's own gap and residual, recomputed in numpy from `face` and `lam`.
Status 2 only where the reference finds no feasible candidate and the oracle's Chebyshev LP says infeasible; status 0 never
there.  What a raw answer may leave out is status 1, up to support_host.HANDBACK_CAPS.  Every test here fails on the parent
commit, which has no plp_nearest.hpp."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import nearest_host as nh  # noqa: E402
import support_host as sh  # noqa: E402


@pytest.fixture(scope="module")
def L(tmp_path_factory):
    return nh.build(tmp_path_factory.mktemp("nearest_host"))


def run_and_check(L, cases, fam, separated):
    counts = [0, 0]
    for case in cases:
        for layout in ("shared", "own"):
            out = nh.run(L, case["A"], case["b"], case[layout][0], case["m"])
            nh.check_case(case, layout, out, counts, separated=separated)
    print("nearest_batch host build, %s: %d of %d problems handed back (%.2f %%)"
          % (fam, counts[1], counts[0], 100.0 * counts[1] / max(counts[0], 1)))
    assert counts[0] > 0 and counts[1] <= nh.HANDBACK_CAPS[fam] * counts[0], counts
    return counts


@pytest.mark.parametrize("fam", nh.FAMILIES)
def test_soak_families_equal_the_reference(L, oracle, fam):
    """The seven soak families at SOAK_SHAPES, B = 10: three normal points, the centre, a point on a facet, one in the normal
    cone of a vertex, one 1e3 extents away and a NaN per polytope, and the points of polytope 0 shared by all."""
    counts = run_and_check(L, nh.cases(oracle, fam), fam, fam in nh.SEPARATED)
    assert counts[0] == 6 * nh.B_CPU * 7 * 2


def test_random_families_equal_the_reference(L, oracle):
    """support_host.family(k): ragged random_hpolytopes per (m, d) of SHAPES, the first 10 of each."""
    run_and_check(L, nh.cases(oracle, "family"), "random", True)


def test_degenerate_polytopes_equal_the_reference(L, oracle):
    """Pyramids, the structured (16, 3) polytopes, the degenerate LPs' polytopes, an empty set, a single point, m = 0."""
    cases = nh.cases(oracle, "degenerate")
    run_and_check(L, cases, "degenerate", False)
    hand = cases[-1]
    out = nh.run(L, hand["A"], hand["b"], hand["own"][0], hand["m"])
    fin = np.isfinite(hand["own"][0]).all(axis=2)
    assert np.all(out["status"][0][fin[0]] == 2) and np.all(out["status"][3][fin[3]] == 2)   # both empty sets, certified
    ok = out["status"][1] == 0
    assert ok.sum() >= 5 and np.allclose(out["x"][1][ok], [0.5, 0.25, 0.0], rtol=0, atol=1e-12)   # the single point
    assert np.all(out["status"][2][fin[2]] == 0) and np.all(out["dist"][2][fin[2]] == 0)           # m = 0: x = p
    assert np.array_equal(out["x"][2][fin[2]], hand["own"][0][2][fin[2]]) and np.all(out["face"][2] == 0)


@pytest.mark.parametrize("fam", ["dup", "flat", "random"])
def test_rows_a_hair_apart_equal_the_exact_reference(L, oracle, fam):
    """m <= 12: the arbiter is the enumeration in exact rational arithmetic on the doubles as stored.  Status 0: dist within
    1e-9 E of the exact one; status 2: no exact candidate is feasible."""
    rng = np.random.default_rng(sh.FAMILY_SEED[fam] + 500)
    n0 = 0
    for (m_max, d) in ((12, 2), (10, 3), (9, 4)):
        A, b, m = sh.family(fam, B=4, rng=rng, shape=(m_max, d))
        X, _ = nh.points_for(oracle, A, b, m, [sh.FAMILY_SEED[fam], m_max])
        X = X[:, [0, 3, 4, 5]]
        out = nh.run(L, A, b, X, m)
        for p in range(4):
            for j in range(4):
                st = out["status"][p, j]
                de, xe = nh.exact_reference(A[p, :m[p]], b[p, :m[p]], X[p, j])
                assert st in (0, 1, 2)
                if st == 2:
                    assert de is None
                if st == 0:
                    n0 += 1
                    E = max(1.0, np.max(np.abs(out["x"][p, j])), np.max(np.abs(X[p, j])))
                    assert de is not None and abs(out["dist"][p, j] - de) <= nh.TOL * E, (p, j, out["dist"][p, j], de)
    assert n0 >= 24


def test_reference_agrees_with_the_exact_one(oracle):
    """The numpy reference against the rational one where nothing is a hair apart."""
    rng = np.random.default_rng(77)
    A, b, m = sh.family("random", B=3, rng=rng, shape=(10, 3))
    X, xc = nh.points_for(oracle, A, b, m, 78)
    rd, rx, rf = nh.reference(A, b, m, X, xc)
    for p in range(3):
        for j in range(7):
            de, xe = nh.exact_reference(A[p], b[p], X[p, j])
            assert rf[p, j] and abs(rd[p, j] - de) <= 1e-12 * max(1.0, de)
            assert np.max(np.abs(rx[p, j] - np.array([float(v) for v in xe]))) <= 1e-11 * max(1.0, np.max(np.abs(X[p, j])))


def test_sanitized_program_runs_every_family(oracle, tmp_path):
    """The stand-alone program of the host build under -fsanitize=address,undefined: once over every family (the records
    written to a file), and once over the polytopes it makes itself; exit 0."""
    exe = nh.build_program(tmp_path)
    recs = []
    for fam in nh.FAMILIES + ("degenerate", "family"):
        for case in nh.cases(oracle, fam):
            recs.append((case["A"], case["b"], case["m"], case["own"][0]))
            recs.append((case["A"], case["b"], case["m"], case["shared"][0]))
    path = str(tmp_path / "records.bin")
    nh.write_records(path, recs)
    for args in ([path], []):
        r = nh.run_program(exe, args)
        assert r.returncode == 0, r.stdout[-2000:]
        assert "inconsistent: 0" in r.stdout


def test_fences(L, oracle):
    """Poisoned rows beyond m[p] and poisoned neighbouring batch members change no output bit."""
    case = nh.cases(oracle, "ragged")[2]
    A, b, m, X = case["A"].copy(), case["b"].copy(), case["m"], case["own"][0]
    ref = nh.run(L, A, b, X, m)
    for p in range(A.shape[0]):
        A[p, m[p]:] = np.nan
        b[p, m[p]:] = -1e300
    got = nh.run(L, A, b, X, m)
    for k in ref:
        assert nh.hb.same_bits(ref[k], got[k]), k
    # one member alone, between poisoned neighbours, equals its answers inside the batch
    for p in (0, 4, 9):
        A3 = np.full((3,) + A.shape[1:], np.nan)
        b3 = np.full((3, A.shape[1]), np.nan)
        A3[1], b3[1] = A[p], b[p]
        X3 = np.full((3,) + X.shape[1:], np.nan)
        X3[1] = X[p]
        one = nh.run(L, A3, b3, X3, np.array([A.shape[1], m[p], A.shape[1]], np.int32))
        for k in ref:
            assert nh.hb.same_bits(ref[k][p], one[k][1]), (k, p)
        assert np.all(one["status"][[0, 2]] == 1)


def test_points_and_faces_are_optional(L, oracle):
    case = nh.cases(oracle, "random")[3]
    full = nh.run(L, case["A"], case["b"], case["shared"][0], case["m"])
    bare = nh.run(L, case["A"], case["b"], case["shared"][0], case["m"], points=False, faces=False)
    assert bare["x"] is None and bare["face"] is None
    assert nh.hb.same_bits(full["dist"], bare["dist"]) and np.array_equal(full["status"], bare["status"])


def test_tiles_and_caps(L):
    """Polytopes per workgroup as support_batch's; a K-chunk is 8 rounds of the lanes a polytope has; the iteration cap."""
    for mm, cap in ((16, 64), (17, 32), (33, 16), (64, 16)):
        for K, v in ((1, 64), (2, 32), (6, 8), (32, 2), (33, 1), (1 << 20, 1)):
            np_ = L.nearest_polytopes_per_group(K, mm)
            assert np_ == min(v, cap)
            assert L.nearest_chunk_points(K, mm) == 8 * (64 // np_)
    assert L.nearest_chunk_points(2 ** 31 - 1, 16) == 64 * -(-(-(-(2 ** 31 - 1) // 64)) // 65535)
    assert L.nearest_polytopes_per_group(4, 65) == 0
    assert [L.nearest_iter_cap(m, d) for m, d in ((0, 1), (16, 3), (64, 4))] == [8, 48, 148]


def test_argument_errors_need_no_library(monkeypatch):
    """Wrong rank of X, d mismatch, B mismatch, K = 0: ValueError; sizes beyond the caps: UnsupportedSize -- all before
    anything of the library is touched."""
    from polytope_amd import _lib, batch

    def no_library(*a, **kw):
        raise AssertionError("the library was touched")
    monkeypatch.setattr(_lib, "load", no_library)
    monkeypatch.setattr(_lib, "context", no_library)
    A, b = np.zeros((3, 6, 2)), np.ones((3, 6))
    for X in (np.zeros(2), np.zeros((2, 3, 4, 2)), np.zeros((4, 3)), np.zeros((3, 4, 3)), np.zeros((2, 4, 2)), np.zeros((0, 2)),
              np.zeros((3, 0, 2))):
        with pytest.raises(ValueError):
            batch.nearest_batch(A, b, X)
    with pytest.raises(ValueError):
        batch.nearest_batch(np.zeros((6, 2)), np.ones(6), np.zeros((4, 2)))
    with pytest.raises(_lib.UnsupportedSize):
        batch.nearest_batch(np.zeros((2, 6, 5)), np.ones((2, 6)), np.zeros((4, 5)))
    with pytest.raises(_lib.UnsupportedSize):
        batch.nearest_batch(np.zeros((2, 65, 3)), np.ones((2, 65)), np.zeros((4, 3)))


def test_resolve_routine_equals_the_reference(oracle):
    """batch._nearest_resolve_one, the host routine behind resolve=True, on problems of every family: it needs no library."""
    from polytope_amd import batch
    n = 0
    for fam in ("random", "dup", "flat"):
        case = nh.cases(oracle, fam)[2]
        P, rd, rx, rf = case["own"]
        N, beta = nh.unit_rows(case["A"], case["b"], case["m"])
        for p in range(0, nh.B_CPU, 2):
            for j in range(7):
                dd, xx, st = batch._nearest_resolve_one(N[p, :case["m"][p]], beta[p, :case["m"][p]], P[p, j], case["xc"][p])[:3]
                if rf[p, j]:
                    E = max(1.0, np.max(np.abs(P[p, j])), np.max(np.abs(rx[p, j])))
                    assert st in (0, 4)
                    if st == 0:
                        n += 1
                        assert abs(dd - rd[p, j]) <= nh.TOL * E
                else:
                    assert st != 0
    assert n >= 80
