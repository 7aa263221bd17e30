"""CPU: the sequential rule of hull_batch (polytope_amd/csrc/plp_hull_enum.hpp: staging, candidates in lexicographic order,
the greedy filter) compiled for the HOST (tests/cabi/hull_enum_host.cpp) and held against what the reference's quickhull()
returned (tests/golden/g30_hull.npz), closed forms, and the argument checks of batch.hull_batch that need no library.

Comparison (tests/hull_host.py: compare), as sets, between rows of unit normal in the distance |dA|_inf + |db| / scale: the
reference's raw rows collapsed at 1e-7 (its simplicial facets repeat a face with more than d points), equal counts, every
reference row within 1e-6 max(1, |b| / scale) of one of ours; the reference's "not fully dimensional" <-> HS_FLAT.
Cases the fixture does not pin are printed with their reason and capped at 2 % of their family.  In the committed file
that is one: case 113 (lattice, 4 points in d = 2 at scale 1e3, all on one line to rounding), on which quickhull() does
not return -- its search for a starting simplex of rank 2 has no end; the rule says HS_FLAT."""
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import hull_host as hh  # noqa: E402
import cap_sweep  # noqa: E402


@pytest.fixture(scope="module")
def L(tmp_path_factory):
    return hh.build(tmp_path_factory.mktemp("hull_host"))


@pytest.fixture(scope="module")
def cases():
    return hh.fixture()


def cube(d):
    return np.array(list(itertools.product([-1.0, 1.0], repeat=d)))


def rows_of(r, p=0):
    """The rows of set p as a dict {rounded (normal, offset): on word}."""
    c = int(r["count"][p])
    return {tuple(np.round(np.r_[r["A"][p, q], r["b"][p, q]], 12) + 0.0): int(r["on"][p, q]) for q in range(c)}


def test_fixture_has_the_cases(cases):
    fams = {}
    for c in cases:
        fams[c["family"]] = fams.get(c["family"], 0) + 1
    assert fams == {"normal": 54, "uniform": 54, "lattice": 54, "sphere": 54, "cube": 9, "cube+inside": 9, "cross": 9, "dup": 9,
                    "flat": 9}
    assert all(c["pinned"] == (c["reason"] == 0) for c in cases)
    assert all(c["ref_kind"] == hh.REF_EMPTY for c in cases if c["family"] == "flat")
    assert {c["scale"] for c in cases} == {1.0, 1e-2, 1e3} and {c["d"] for c in cases} == {2, 3, 4}


def test_host_build_against_the_reference(L, cases):
    results = []
    for c in cases:
        r = hh.run(L, c["X"][None])
        cnt = int(r["count"][0])
        X, d = c["X"], c["d"]
        ext = np.abs(X - (X.min(0) + X.max(0)) / 2).max()
        for q in range(cnt):
            a, beta, sub = r["A"][0, q], r["b"][0, q], r["basis"][0, q]
            # a unit normal, every point on its right side, the basis increasing and on the facet, `on` = the points on it
            assert abs(np.linalg.norm(a) - 1.0) < 1e-14
            res = (X @ a - beta) / ext
            assert np.all(res <= 2e-9) and np.all(np.diff(sub) > 0)
            assert hh.bits(r["on"][0, q]) >= set(sub.tolist())
            assert set(np.nonzero(np.abs(res) <= 1e-10)[0].tolist()) <= hh.bits(r["on"][0, q]) <= set(np.nonzero(np.abs(res) <= 1e-8)[0].tolist())
        assert np.all(np.isnan(r["A"][0, cnt:])) and np.all(np.isnan(r["b"][0, cnt:]))
        assert np.all(r["on"][0, cnt:] == 0) and np.all(r["basis"][0, cnt:] == -1)
        results.append((r["A"][0], r["b"][0], cnt, r["status"][0]))
    assert hh.check_cases(cases, results, "host build") <= 1


def test_every_status_and_the_slots_beyond_count(L):
    X = np.zeros((5, 9, 3))
    X[0, :8] = cube(3)                      # OK
    X[1, :8] = cube(3)
    X[1, :, 2] = 0.5                        # FLAT: one plane
    X[2, :] = 1.25                          # FLAT: one point nine times (s = 0)
    X[3, :8] = cube(3)                      # FLAT by n: three points
    X[4, :8] = cube(3) * 1e-3 + 7.0         # OK
    n = np.array([8, 8, 9, 3, 8], np.int32)
    r = hh.run(L, X, n, f_max=7)
    assert r["status"].tolist() == [hh.HS_OK, hh.HS_FLAT, hh.HS_FLAT, hh.HS_FLAT, hh.HS_OK]
    assert r["count"].tolist() == [6, 0, 0, 0, 6]
    r5 = hh.run(L, X, n, f_max=5)
    assert r5["status"].tolist() == [hh.HS_OVERFLOW, hh.HS_FLAT, hh.HS_FLAT, hh.HS_FLAT, hh.HS_OVERFLOW]
    assert r5["count"].tolist() == [5, 0, 0, 0, 5]
    for res in (r, r5):
        for p in range(5):
            c = res["count"][p]
            assert np.all(np.isfinite(res["A"][p, :c])) and np.all(np.isfinite(res["b"][p, :c])) and np.all(res["on"][p, :c] != 0)
            assert np.all(np.isnan(res["A"][p, c:])) and np.all(np.isnan(res["b"][p, c:]))
            assert np.all(res["on"][p, c:] == 0) and np.all(res["basis"][p, c:] == -1)
    # exactly f_max facets is not an overflow; a keep mask that leaves three corners is flat; without the basis
    assert hh.run(L, X[:1], n[:1], f_max=6)["status"][0] == hh.HS_OK
    assert hh.run(L, X[:1], n[:1], keep=np.array([0b1011], np.uint64))["status"][0] == hh.HS_FLAT
    nb = hh.run(L, X, n, f_max=7, basis=False)
    assert nb["basis"] is None and hh.same_result(nb, r, basis=False) is None


def test_closed_forms(L):
    # d = 1: x <= max and -x <= -min, whatever lies between
    x = np.array([0.5, -3.0, 2.0, 7.25, 1.0])
    r = hh.run(L, x.reshape(1, 5, 1))
    assert r["status"][0] == hh.HS_OK and rows_of(r) == {(1.0, 7.25): 1 << 3, (-1.0, 3.0): 1 << 1}
    # the square, the cube and the 4-cube: 2 d rows +-e_k x <= 1, each with exactly the 2^(d - 1) corners of that face
    for d in (2, 3, 4):
        P = cube(d)
        r = hh.run(L, P[None])
        want = {}
        for k in range(d):
            for sgn in (1.0, -1.0):
                want[tuple(np.r_[sgn * np.eye(d)[k], 1.0] + 0.0)] = int(hh.keep_word(P[:, k] == sgn))
        assert r["status"][0] == hh.HS_OK and r["count"][0] == 2 * d and rows_of(r) == want
        assert all(len(hh.bits(w)) == 2 ** (d - 1) for w in want.values())
        # the cross-polytope: 2^d rows sign.x <= 1 (unit normals: sign / sqrt(d))
        r = hh.run(L, np.vstack([np.eye(d), -np.eye(d)])[None])
        got = rows_of(r)
        assert r["status"][0] == hh.HS_OK and len(got) == 2 ** d
        assert {k[:d] for k in got} == {tuple(np.round(np.array(sg) / np.sqrt(d), 12)) for sg in itertools.product([-1.0, 1.0], repeat=d)}
        assert all(abs(k[d] - 1 / np.sqrt(d)) < 1e-12 and len(hh.bits(w)) == d for k, w in got.items())
    # a point at the centre of a face of the cube appears in that facet's `on` and changes no row
    P = cube(3)
    base = hh.run(L, P[None])
    more = hh.run(L, np.vstack([P, [[1.0, 0.0, 0.0]]])[None], f_max=12)
    got, want = rows_of(more), rows_of(base)
    assert more["status"][0] == hh.HS_OK and more["count"][0] == 6 and set(got) == set(want)
    for key, w in want.items():
        assert got[key] == w | ((1 << 8) if key[0] == 1.0 else 0)


def test_overflow_keeps_the_first_facets(L):
    rng = np.random.default_rng(3)
    X = rng.standard_normal((6, 14, 3))
    X[3] = rng.integers(-2, 3, (14, 3))
    full = hh.run(L, X)
    assert np.all(full["status"] == hh.HS_OK) and full["count"].min() > 4
    cut = hh.run(L, X, f_max=4)
    assert np.all(cut["status"] == hh.HS_OVERFLOW) and np.all(cut["count"] == 4)
    assert hh.same_bits(cut["A"], full["A"][:, :4]) and hh.same_bits(cut["b"], full["b"][:, :4])
    assert np.array_equal(cut["on"], full["on"][:, :4]) and np.array_equal(cut["basis"], full["basis"][:, :4])


def test_cap_sweep_overflow_in_a_later_round(L):
    """Every cap from 1 to the full count + 1 on two sets whose candidates take two rounds of 64 in the kernel: the
    12-gon's last facet is the edge (10, 11), subset 65 of 66; the last facet of the nine points comes from a subset of rank
    >= 64 too.  (The host build has no rounds: this pins the list the kernel is held against in tests/test_hull_gpu.py.)"""
    gon, pts = cap_sweep.hull_members()
    whole, full = cap_sweep.check_hull(gon, lambda X, k: hh.run(L, X, f_max=k))
    assert full == 12 and whole["basis"][0, 11].tolist() == [10, 11]
    assert np.allclose(whole["b"][0, :12], np.cos(np.pi / 12)) and all(len(hh.bits(w)) == 2 for w in whole["on"][0, :12])
    whole, full = cap_sweep.check_hull(pts, lambda X, k: hh.run(L, X, f_max=k))
    assert cap_sweep.subset_rank(whole["basis"][0, full - 1].tolist(), 9) >= 64 > cap_sweep.subset_rank(whole["basis"][0, 0].tolist(), 9)


def test_shift_and_power_of_two_scale_change_no_bit(L):
    """Points on a dyadic grid, a dyadic shift and a power of two: every sum is exact, so the staged points are the same
    numbers and A, on and basis the same bits; b follows the map."""
    rng = np.random.default_rng(5)
    for d in (1, 2, 3, 4):
        X = rng.integers(-64, 65, (8, 13, d)) / 16.0
        X[5] = rng.integers(-2, 3, (13, d))
        n = rng.integers(d + 1, 14, size=8).astype(np.int32)
        keep = np.array([hh.keep_word(np.r_[np.ones(d + 1, bool), rng.random(63 - d) < 0.8]) for _ in range(8)])
        base = hh.run(L, X, n, keep)
        assert (base["status"] == hh.HS_OK).sum() >= 6
        for scale, shift in ((1.0, 16.0), (2.0 ** -7, 0.0), (2.0 ** 9, -40.0)):
            t = shift * np.arange(1, d + 1) / 4.0
            moved = hh.run(L, (X + t) * scale, n, keep)
            assert hh.same_bits(moved["A"], base["A"]) and np.array_equal(moved["on"], base["on"])
            assert np.array_equal(moved["basis"], base["basis"]) and np.array_equal(moved["status"], base["status"])
            want = (base["b"] + base["A"] @ t) * scale
            ok = ~np.isnan(want)
            assert np.allclose(moved["b"][ok], want[ok], rtol=1e-13, atol=1e-13 * scale) and np.array_equal(np.isnan(moved["b"]), ~ok)


def test_stand_alone_program_under_sanitizers(tmp_path, cases):
    """The host build with a main() of its own under -fsanitize=address,undefined: the fixture's point sets packed into one
    ragged batch per dimension, run with every point, with a keep mask with holes, with f_max = 3 and without the basis
    (nothing is loaded into this interpreter)."""
    sets = [c["X"] for c in cases] + [np.array([[0.5], [2.0], [-1.0]]), np.zeros((0, 2)), np.ones((64, 3))]
    sets.append(np.random.default_rng(1).standard_normal((64, 4)))
    path = tmp_path / "points.bin"
    with open(path, "wb") as f:
        f.write(np.int32(len(sets)).tobytes())
        for X in sets:
            f.write(np.array(X.shape, np.int32).tobytes())
            f.write(np.ascontiguousarray(X, dtype=np.float64).tobytes())
    prog = hh.build_program(tmp_path)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    out = subprocess.run([prog, str(path)], capture_output=True, text=True, env=env, timeout=300)
    print(out.stdout)
    assert out.returncode == 0, (out.returncode, out.stdout[-2000:], out.stderr[-4000:])
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, out.stderr[-4000:]
    assert "inconsistent: 0" in out.stdout and "%d point sets" % len(sets) in out.stdout


def test_argument_errors_need_no_library():
    from polytope_amd import batch
    X = np.zeros((2, 6, 3))
    for bad in (lambda: batch.hull_batch(np.zeros((6, 3))),
                lambda: batch.hull_batch(np.zeros((2, 12, 5))),
                lambda: batch.hull_batch(np.zeros((2, 65, 3))),
                lambda: batch.hull_batch(X, n=np.zeros(3, np.int32)),
                lambda: batch.hull_batch(X, f_max=0),
                lambda: batch.hull_batch(X, f_max=-4),
                lambda: batch.hull_batch(X, f_max=2.5)):
        with pytest.raises(ValueError):
            bad()
    import polytope_amd as pa
    assert pa.hull_batch is batch.hull_batch
    assert (batch.HS_OK, batch.HS_OVERFLOW, batch.HS_FLAT) == (hh.HS_OK, hh.HS_OVERFLOW, hh.HS_FLAT) == (0, 1, 2)
    assert [hh.fmax_for(d, n) for d in (1, 2, 3, 4) for n in (0, 5, 64)] == [batch._extreme_vmax(d, n) for d in (1, 2, 3, 4) for n in (0, 5, 64)]
