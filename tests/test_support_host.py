"""CPU: the per-LP function of support_kernel (polytope_amd/csrc/plp_support.hpp: rows staged as a_i / beta_i, the lane
walk, the end check, the status mapping) compiled for the HOST (tests/cabi/support_host.cpp) and held against the oracle's
simplex, and the argument checks of batch.support_batch that need no library.

Tolerance (tests/support_host.py: check_against_oracle): status equal to oracle.lp_solve's; where it is 0,
|h - (-fun)| <= 1e-9 max(1, |h|); x is not compared (ties have no unique vertex) but A x <= b + 1e-9 and
|c.x - h| <= 1e-12 max(1, |h|).  On the soak families (scripts/soak_lane.py: make) and the degenerate cases the first two
are relative to the extent max(1, |h|, |x_oracle|_max), the rule of tests/test_verify_host.py.

What a raw answer may leave out is status 1, up to a cap (support_host.HANDBACK_CAPS); a status 0 is the optimum.  The
parent of the commit that added the optimality end check failed test_the_lps_the_soak_found on all four LPs (h = 1.2492
for 2.0904, 0.70572 for 1.0469, 1.897860 for 1.897861, 3.903764 for 3.903765: feasible points, not optimal)."""
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


def soak_family_case(O, fam, seed=None, shapes=sh.SOAK_SHAPES, translate=0.0):
    """The cases of a soak family (support_host.soak_cases) or of "degenerate", with their oracle answers, once per session."""
    if fam == "degenerate":
        return sh.memo(("degenerate",), lambda: sh.degenerate_cases(O))
    seed = sh.FAMILY_SEED[fam] if seed is None else seed
    return sh.memo(("soak", fam, seed, shapes, translate), lambda: sh.soak_cases(O, fam, seed, shapes, translate=translate))


def run_and_check(L, cases, fam):
    """Both layouts of C of every case through the host build and check_case; the share handed back, printed and capped."""
    counts = [0, 0]
    for case in cases:
        for layout in ("shared", "own"):
            h, x, st = sh.run_case(L, case, layout)
            sh.check_case(case, layout, h, x, st, counts)
    print("support_batch host build, %s: %d of %d LPs handed back (%.2f %%)" % (fam, counts[1], counts[0], 100.0 * counts[1] / max(counts[0], 1)))
    assert counts[0] > 0 and counts[1] <= sh.HANDBACK_CAPS[fam] * counts[0], counts
    return counts


@pytest.mark.parametrize("fam", sh.FAMILIES)
def test_soak_families_equal_the_oracle(L, oracle, fam):
    """The seven soak families at (16, 1), (17, 2), (16, 3), (64, 3), (32, 4), (48, 4) -- walk3 at d = 1, 2, 3, walk4, every
    row-slot count -- B = 30 each: 7 random directions + -e_i shared, the tie directions (a row's normal: a whole facet is
    optimal, on `dup` a hair row's; the sum of two neighbouring normals; -a_i) and two random ones per polytope.  A polytope
    without a Chebyshev centre of radius > 0 gets a NaN centre and comes back as status 1 throughout."""
    cases = soak_family_case(oracle, fam)
    counts = run_and_check(L, cases, fam)
    assert counts[0] >= 0.7 * sum(c["A"].shape[0] * (c["shared"][0].shape[0] + 9) for c in cases)
    if fam == "flat":
        assert any(not np.isfinite(c["xc"]).all() for c in cases)


@pytest.mark.parametrize("fam", sh.FAMILIES)
def test_soak_families_translated(L, oracle, fam):
    """b += A t, |t| = 1e3, at (32, 4) and (16, 3): beta = b - a.xc cancels three digits and h is held to 1e-9 of THAT extent."""
    run_and_check(L, soak_family_case(oracle, fam, seed=sh.FAMILY_SEED[fam] + 100, shapes=((32, 4), (16, 3)), translate=1e3), fam)


@pytest.mark.parametrize("seed", [7, 8, 9, 10])
def test_dup_family_of_the_first_soak(L, oracle, seed):
    """`dup` on the generator stream that found status-0 answers that were feasible and not optimal (seeds 7 and 8; 9 and
    10 were clean): every answer that is not handed back is the oracle's."""
    run_and_check(L, soak_family_case(oracle, "dup", seed=seed, shapes=sh.FOUND_SHAPES), "dup")


@pytest.mark.parametrize("seed,shape,p,j", sh.FOUND)
def test_the_lps_the_soak_found(L, oracle, seed, shape, p, j):
    """The four LPs by name, from the stream and from tests/golden/found/support/dup.npz (the polytope, its directions, the
    oracle's h as recorded there): status 1, or the optimum."""
    case = soak_family_case(oracle, "dup", seed=seed, shapes=sh.FOUND_SHAPES)[sh.FOUND_SHAPES.index(shape)]
    C_, ost, oh, ox = case["shared"]
    z = np.load(os.path.join(ROOT, "tests", "golden", "found", "support", "dup.npz"))
    key = "s%d_m%d_p%d" % (seed, shape[0], p)
    assert np.array_equal(z["A_" + key], case["A"][p]) and np.array_equal(z["b_" + key], case["b"][p])
    assert np.array_equal(z["C_" + key], C_) and ost[p, j] == 0
    assert abs(z["h_" + key][j] - oh[p, j]) <= 1e-9 * max(1.0, abs(oh[p, j]))
    h, x, st = sh.run(L, z["A_" + key][None], z["b_" + key][None], z["C_" + key], z["xc_" + key][None])
    assert st[0, j] in (0, 1)
    if st[0, j] == 0:
        assert abs(h[0, j] - oh[p, j]) <= 1e-9 * max(1.0, abs(h[0, j]), ox[p, j]), (h[0, j], oh[p, j])
    # ... and every other direction of that polytope
    ok = st[0] == 0
    assert np.array_equal(st[0][st[0] != 1], ost[p][st[0] != 1])
    assert np.all(np.abs(h[0][ok] - z["h_" + key][ok]) <= 1e-9 * np.maximum(1.0, np.fmax(np.abs(h[0][ok]), ox[p][ok])))


OFF = sh.oracle_off_fixture()


@pytest.mark.parametrize("i", range(len(OFF)), ids=[f[0] for f in OFF])
def test_lps_on_which_the_oracle_is_off(L, oracle, i):
    """The 54 LPs of the `dup` soak (seeds 1000 .. 1199 and 14) on which the oracle is more than 1e-9 of the extent from the
    exact optimum (it reads entries <= 1e-9 as zero, accepts points 1e-9 outside a row, calls a vertex 1e9 away unbounded):
    the reference here is support_host.exact_support, rational arithmetic on the stored doubles -- recomputed, equal to the
    recorded one -- and the host build's answer is status 1 or within 1e-9 of the extent of THAT; the oracle is not."""
    name, A, b, c, xc, he, ext = OFF[i]
    hx, xe = sh.exact_support(A, b, c, xc)
    assert float(hx) == he and max(1.0, abs(he), max(abs(float(v)) for v in xe)) == ext
    so, xo, fo, _ = oracle.lp_solve(-c, A, b)
    assert so == 3 or abs(-fo - he) > 1e-9 * max(1.0, abs(fo), float(np.max(np.abs(xo)))), "the oracle is right here now: drop the case"
    h, x, st = sh.run(L, A[None], b[None], c[None], xc[None])
    assert st[0, 0] in (0, 1)
    if st[0, 0] == 0:
        assert abs(h[0, 0] - he) <= 1e-9 * ext, (h[0, 0], he)
        assert np.max(A @ x[0, 0] - b) <= 1e-9 * ext and abs(c @ x[0, 0] - h[0, 0]) <= 1e-12 * max(1.0, abs(h[0, 0]))


def test_exact_support_is_a_simplex(oracle):
    """The arbiter against the oracle where nothing is a hair apart: `random` and `unbounded` at (16, 3) and (12, 2), every LP --
    unbounded where the oracle says 3, the oracle's h to 1e-12 elsewhere."""
    for fam, seed in (("random", 1), ("unbounded", 3)):
        for case in soak_family_case(oracle, fam, seed=seed, shapes=((16, 3), (12, 2))):
            C_, ost, oh, _ = case["shared"]
            for p in range(0, 30, 3):
                for j in range(C_.shape[0]):
                    he, _ = sh.exact_support(case["A"][p, :case["m"][p]], case["b"][p, :case["m"][p]], C_[j], case["xc"][p])
                    assert (he is None) == (ost[p, j] == 3)
                    assert he is None or abs(float(he) - oh[p, j]) <= 1e-12 * max(1.0, abs(oh[p, j]))


def test_degenerate_vertices_equal_the_oracle(L, oracle):
    """Pyramids (m - d - 1 facets through one apex, some 1e-5 apart), the structured (16, 3) polytopes and the degenerate
    LPs' polytopes at d <= 4: 9 random directions + -e_i, the tie directions, the LP's own cost."""
    run_and_check(L, soak_family_case(oracle, "degenerate"), "degenerate")


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


def test_sanitized_program_runs(tmp_path):
    """The stand-alone program of the host build (-DSUPPORT_HOST_MAIN: the polytopes it makes itself, every d and row-slot
    count, interior / boundary / NaN centres) under -fsanitize=address,undefined: exit 0, every status consistent."""
    import subprocess
    r = subprocess.run([sh.build_program(tmp_path)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert r.returncode == 0, r.stdout[-2000:]
    assert "inconsistent: 0" in r.stdout


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
