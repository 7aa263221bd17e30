"""CPU: the sequential rule of volume_exact_batch (polytope_amd/csrc/plp_volume_exact.hpp: staging, chains, the parallel
tests with ownership, lines, sums in index order) compiled for the HOST (tests/cabi/volume_exact_host.cpp) and held against
closed forms, against its own identities (the facet areas weighted by their normals add up to 0) and against the reference
(tests/golden/g30_volume_exact.npz: its Monte-Carlo volume() and scipy's hull volume of its extreme()); and the argument
checks of batch.volume_exact_batch that need no library.

The public call's steps are taken here on the scipy backend of this package: FLAT where is_fulldim says no, UNBOUNDED where
a side of bounding_box is infinite, else the rows reduce() keeps, about the centre of the box at half its longest side."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import volume_exact_host as vh  # noqa: E402

REL = 1e-13


@pytest.fixture(scope="module")
def L(tmp_path_factory):
    return vh.build(tmp_path_factory.mktemp("volume_exact_host"))


@pytest.fixture(scope="module")
def cases():
    return vh.fixture()


def public_on_scipy(L, A, b):
    """(volume, status, rows A, b the rule ran on, areas) as the public call decides them, on the scipy backend."""
    import polytope_amd as pa
    assert pa.solvers.default_solver == "scipy"
    P = pa.Polytope(A.copy(), b.copy())
    if not pa.is_fulldim(P):
        return 0.0, vh.VS_FLAT, None, None, None
    lb, ub = (np.asarray(v, float).ravel() for v in P.bounding_box)
    if not (np.all(np.isfinite(lb)) and np.all(np.isfinite(ub))):
        return math.inf, vh.VS_UNBOUNDED, None, None, None
    R = pa.reduce(P)
    RA, Rb = np.asarray(R.A, float), np.asarray(R.b, float).ravel()
    vol, area, status = vh.one(L, RA, Rb, xc=0.5 * (lb + ub), scale=0.5 * float((ub - lb).max()))
    return vol, status, RA, Rb, area


def named(A, b):
    """The variations of a named polytope that leave its volume alone -> [(what, A, b, kwargs)]."""
    d = A.shape[1]
    rng = np.random.default_rng(5)
    perm = rng.permutation(len(A))
    A2, b2 = np.vstack([A, A]), np.r_[b, b]
    perm2 = rng.permutation(len(A2))
    off = np.arange(1.0, d + 1)      # the origin is 1 .. d units away from the centre along the axes: outside all of them
    far = 1e3 * np.arange(1.0, d + 1)
    return [("as given", A, b, {}), ("rows permuted", A[perm], b[perm], {}), ("every row twice", A2, b2, {}),
            ("every row twice, permuted", A2[perm2], b2[perm2], {}), ("reference point outside", A, b + A @ off, {}),
            ("shifted by 1e3, xc and scale", A, b + A @ far, dict(xc=far, scale=2.0)),
            ("shifted by 1e3, xc off centre", A, b + A @ far, dict(xc=far + 0.25, scale=0.5))]


def test_closed_forms(L):
    worst = 0.0
    for name, A, b, V in vh.closed_forms():
        for what, Av, bv, kw in (named(A, b) if "simplex" not in name else named(A, b)[:4]):
            vol, area, status = vh.one(L, Av, bv, **kw)
            err = abs(vol - V) / V
            worst = max(worst, err)
            print("%-22s %-32s %.17g  %.1e" % (name, what, vol, err))
            assert status == vh.VS_OK and err <= REL, (name, what, vol, V)
            if A.shape[1] > 1:   # the areas of a closed surface, weighted by their unit normals, cancel
                un = Av / np.linalg.norm(Av, axis=1)[:, None]
                assert np.abs(area @ un).max() <= 1e-12 * area.sum(), (name, what)
    print("worst relative error %.2e" % worst)


def test_cross_polytope_4_needs_ownership(L):
    """Every edge of the 4-d cross-polytope lies in four facets; counted once per facet that induces it inside a 2-face the
    volume comes out as 4/3."""
    A, b = vh.cross(4)
    vol, area, status = vh.one(L, A, b)
    assert status == vh.VS_OK and abs(vol - 2.0 / 3.0) <= REL * 2.0 / 3.0
    assert np.allclose(area, 1.0 / 3.0, rtol=1e-13, atol=0)   # 16 regular tetrahedra of edge sqrt(2)
    A24, b24 = vh.cell24()
    assert abs(vh.one(L, A24, b24)[0] - 2.0) <= REL * 2.0


def test_areas_of_named_polytopes(L):
    A, b = vh.cube(3, 0.75)
    assert np.array_equal(vh.one(L, A, b)[1], np.full(6, 2.25))
    A2, b2 = np.vstack([A, A]), np.r_[b, b]
    assert np.array_equal(vh.one(L, A2, b2)[1], np.r_[np.full(6, 2.25), np.zeros(6)])   # the first of two equal rows owns the facet
    v, a, s = vh.one(L, np.array([[2.0], [-1.0], [1.0], [2.0]]), np.array([3.0, 0.25, 9.0, 3.0]))
    assert (v, s) == (1.75, vh.VS_OK) and np.array_equal(a, [1.0, 1.0, 0.0, 0.0])


def test_statuses(L):
    A, b = vh.cube(3)
    Z = np.concatenate([A, np.zeros((1, 3))])
    assert vh.one(L, Z, np.r_[b, -1.0])[::2] == (0.0, vh.VS_EMPTY)
    assert vh.one(L, Z, np.r_[b, np.nan])[::2] == (0.0, vh.VS_EMPTY)
    assert vh.one(L, Z, np.r_[b, 0.0])[::2] == vh.one(L, A, b)[::2] and abs(vh.one(L, A, b)[0] - 8.0) <= 8 * REL
    # a prism without its ends; a slab; fewer rows than dimensions; no rows at all
    assert vh.one(L, A[[0, 1, 3, 4]], b[:4])[::2] == (math.inf, vh.VS_UNBOUNDED)
    assert vh.one(L, A[[0, 3]], b[:2])[::2] == (math.inf, vh.VS_UNBOUNDED)
    assert vh.one(L, A[:2], b[:2])[::2] == (math.inf, vh.VS_UNBOUNDED)
    assert vh.one(L, A, b, m=0)[::2] == (math.inf, vh.VS_UNBOUNDED)
    assert vh.one(L, A, b, keep=np.uint64(0))[::2] == (math.inf, vh.VS_UNBOUNDED)
    # empty and flat sets have volume 0 and are no error
    assert vh.one(L, A, np.r_[1.0, 1, 1, -2, 1, 1])[::2] == (0.0, vh.VS_OK)
    assert vh.one(L, A[[0, 3]], np.r_[1.0, -2.0])[::2] == (0.0, vh.VS_OK)
    assert vh.one(L, A, np.r_[1.0, 1, 1, -1, 1, 1])[::2] == (0.0, vh.VS_OK)
    # a keep word with holes: the rows that are left are the polytope
    A8 = np.concatenate([A, np.array([[1.0, 1, 1], [1, 1, 1]])])
    b8 = np.r_[b, 0.0, 2.0]   # row 6 (dropped) would cut the cube in half, row 7 cuts a corner of volume 1 / 6 off
    vol, area, status = vh.one(L, A8, b8, keep=np.uint64(0b111111 | (1 << 7)))
    assert status == vh.VS_OK and abs(vol - (8.0 - 1.0 / 6.0)) <= 8 * REL and area[6] == 0.0
    assert abs(area[7] - math.sqrt(3) / 2) <= 1e-13
    # sizes the kernel does not take
    assert L.volume_exact_host(1, 65, 3, None, None, None, None, None, None, None, None, None) == 2
    assert L.volume_exact_host(1, 6, 5, None, None, None, None, None, None, None, None, None) == 2
    assert L.volume_exact_host(0, 6, 3, None, None, None, None, None, None, None, None, None) == 2


# ------------------------------------------------------------------------------------------------ the eps sweep
def sweep_polytopes():
    """Six polytopes, d = 2, 3, 4: the cube and a random polytope inside a box, each with the facet to tilt and a point of
    that facet (the mean of its vertices)."""
    from scipy.spatial import HalfspaceIntersection
    out = []
    rng = np.random.default_rng(17)
    for d in (2, 3, 4):
        A, b = vh.cube(d)
        out.append(("cube %d" % d, A, b, 0, np.eye(d)[0]))
        G = rng.standard_normal((4 * d, d))
        G /= np.linalg.norm(G, axis=1)[:, None]
        A, b = np.vstack([A, G]), np.r_[b, 0.8 + 0.4 * rng.random(4 * d)]
        V = HalfspaceIntersection(np.c_[A, -b], np.zeros(d)).intersections
        on = [np.abs(V @ A[i] - b[i]) <= 1e-9 for i in range(len(A))]
        i = max(range(2 * d, len(A)), key=lambda k: on[k].sum())
        assert on[i].sum() >= d
        out.append(("random %d" % d, A, b, i, V[on[i]].mean(0)))
    return out


def test_eps_sweep(L):
    """A copy of one facet's row, tilted by eps about a point of the facet, is added: the volume moves by at most
    eps + 1e-15 / eps of itself (eps: what the tilted row cuts off; 1e-15 / eps: the conditioning of crossing two rows eps
    apart; the host build's worst is 7.4e-17 / eps, the prototype of the rule had 5e-17 / eps)."""
    worst = {}
    for name, A, b, i, c in sweep_polytopes():
        d = A.shape[1]
        V0 = vh.one(L, A, b)[0]
        rng = np.random.default_rng(3)
        for eps in 10.0 ** np.arange(-13.0, -3.5, 0.5):
            for _ in range(4):
                t = rng.standard_normal(d)
                t -= (t @ A[i]) * A[i] / (A[i] @ A[i])
                t /= np.linalg.norm(t)
                a2 = math.cos(eps) * A[i] / np.linalg.norm(A[i]) + math.sin(eps) * t
                vol, _, status = vh.one(L, np.vstack([A, a2]), np.r_[b, a2 @ c])
                err = abs(vol - V0) / V0
                worst[eps] = max(worst.get(eps, 0.0), (err - eps) * eps)
                assert status == vh.VS_OK and err <= eps + 1e-15 / eps, (name, eps, vol, V0, err)
    print("worst (error - eps) * eps over the sweep: %.2e (the bound is 1e-15)" % max(worst.values()))


# ------------------------------------------------------------------------------------------------ the fixture
def test_fixture_has_the_cases(cases):
    fams = {}
    for c in cases:
        fams[c["family"]] = fams.get(c["family"], 0) + 1
    assert fams == {"random": 24, "ragged": 24, "dup": 32, "scaled": 24, "flat": 40, "lattice": 24}
    assert sum(c["unbounded"] for c in cases) > 0 and sum(c["flat"] for c in cases) > 0
    assert all(np.isfinite(c["vol_mc"]) for c in cases if not (c["flat"] or c["unbounded"]))


def test_host_build_against_the_reference(L, cases):
    results = []
    for c in cases:
        vol, status, RA, Rb, area = public_on_scipy(L, c["A"], c["b"])
        if status == vh.VS_OK and c["d"] > 1:   # a closed surface, whatever qhull says
            un = RA / np.linalg.norm(RA, axis=1)[:, None]
            assert np.abs(area @ un).max() <= 1e-12 * area.sum(), (c["index"], c["family"])
        results.append((vol, status))
    vh.check_cases(cases, results, "host build")


def test_stand_alone_program_under_sanitizers(tmp_path, cases):
    """The host build with a main() of its own under -fsanitize=address,undefined on the fixture's rows (nothing is loaded
    into this interpreter)."""
    path = tmp_path / "rows.bin"
    with open(path, "wb") as f:
        f.write(np.int32(len(cases)).tobytes())
        for c in cases:
            f.write(np.array(c["A"].shape, np.int32).tobytes())
            f.write(np.ascontiguousarray(c["A"]).tobytes())
            f.write(np.ascontiguousarray(c["b"]).tobytes())
    prog = vh.build_program(tmp_path)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    out = subprocess.run([prog, str(path)], capture_output=True, text=True, env=env, timeout=300)
    print(out.stdout)
    assert out.returncode == 0, (out.returncode, out.stdout[-2000:], out.stderr[-4000:])
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, out.stderr[-4000:]
    assert "inconsistent: 0" in out.stdout


def test_argument_errors_need_no_library():
    import polytope_amd as pa
    from polytope_amd import batch
    A, b = np.zeros((2, 6, 3)), np.zeros((2, 6))
    for bad in (lambda: batch.volume_exact_batch(np.zeros((6, 3)), np.zeros(6)),
                lambda: batch.volume_exact_batch(A, np.zeros((2, 5))),
                lambda: batch.volume_exact_batch(A, np.zeros(12)),
                lambda: batch.volume_exact_batch(np.zeros((2, 12, 5)), np.zeros((2, 12))),
                lambda: batch.volume_exact_batch(np.zeros((2, 65, 3)), np.zeros((2, 65))),
                lambda: batch.volume_exact_batch(A, b, m=np.zeros(3, np.int32))):
        with pytest.raises(ValueError):
            bad()
    assert pa.volume_exact_batch is batch.volume_exact_batch and pa.volume_exact is pa.polytope.volume_exact
    assert (batch.VS_OK, batch.VS_UNBOUNDED, batch.VS_EMPTY, batch.VS_FLAT) == (0, 1, 2, 3)
    empty = batch.volume_exact_batch(np.zeros((0, 6, 3)), np.zeros((0, 6)))
    assert empty["volume"].shape == (0,) and empty["area"].shape == (0, 6) and empty["status"].dtype == np.int32
    box = pa.box2poly([[0.0, 1.0], [0.0, 2.0]])
    with pytest.raises(Exception, match="regions"):
        pa.volume_exact(pa.Region([box, box]))
