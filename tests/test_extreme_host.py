"""CPU: the sequential rule of extreme_batch (polytope_amd/csrc/plp_extreme.hpp: staging, candidates in lexicographic
order, the greedy filter) compiled for the HOST (tests/cabi/extreme_host.cpp) and held against what the reference's
extreme() returned (tests/golden/g29_extreme.npz), and the argument checks of batch.extreme_batch that need no library.

The public call's steps are taken here by the oracle: `keep` from oracle.reduce; FLAT where oracle.cheby does not end with
r > 1e-7, UNBOUNDED where a side of oracle.bounding_box is not finite.  Comparison (tests/extreme_host.py: compare), as
sets: the reference's rows collapsed at 1e-7 of the extent E = max(1, |V|_inf), equal counts, every vertex within 1e-8 E of
one of the other side's; FLAT / UNBOUNDED is right where the reference returned None, raised or wrote non-finite rows.
The reference is not repeatable on such input (inf in one call, finite rows of magnitude 2^56 in the next, for the same 7
rows in d = 4), so the fixture records five calls per case: FLAT / UNBOUNDED is right only where one of them had no
answer, vertices only where one of them had, and then against that call's rows.  The calls disagree on cases 186 and 191
(ragged, unbounded); everywhere else there is one right answer.
Cases the fixture does not pin (the reference's rows hold two vertices 1e-10 .. 1e-7 of the extent apart: one vertex to
the collapse, two to an enumeration) are printed with their reason and capped at
10 % of the flat family, none elsewhere."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import extreme_host as xh  # noqa: E402
import cap_sweep  # noqa: E402


@pytest.fixture(scope="module")
def L(tmp_path_factory):
    return xh.build(tmp_path_factory.mktemp("extreme_host"))


@pytest.fixture(scope="module")
def cases():
    return xh.fixture()


def oracle_verdict(O, A, b):
    """(status or None, keep bool[m]) as the public call decides them, by the oracle."""
    st, r, _ = O.cheby(A, b)
    if st != 0 or not r > xh.ABS_TOL:
        return xh.XS_FLAT, None
    lb, ub, _ = O.bounding_box(A, b)
    if not (np.all(np.isfinite(lb)) and np.all(np.isfinite(ub))):
        return xh.XS_UNBOUNDED, None
    return None, np.asarray(O.reduce(A, b)["keep"], bool)


def test_fixture_has_the_cases(cases):
    fams = {}
    for c in cases:
        fams[c["family"]] = fams.get(c["family"], 0) + 1
    assert fams == {"random": 16, "scaled": 16, "lattice": 16, "dup": 48, "ragged": 48, "flat": 48, "unbounded": 48, "named": 8}
    assert all(c["pinned"] == (c["reason"] == 0) for c in cases)


def test_unrank_is_the_lexicographic_order(L):
    for d in (1, 2, 3, 4):
        assert L.extreme_unrank_mismatches(d) == 0


def test_host_build_against_the_reference(L, oracle, cases):
    results = []
    for c in cases:
        verdict, keep = oracle_verdict(oracle, c["A"], c["b"])
        if verdict is not None:
            results.append((np.zeros((0, c["d"])), 0, verdict))
            continue
        V, count, basis, status = xh.run(L, c["A"][None], c["b"][None], keep=np.array([xh.keep_word(keep)]))
        # the basis is what the vertex lies on: d kept rows of the input, increasing, tight at the vertex
        for q in range(count[0]):
            rows = basis[0, q]
            assert np.all(np.diff(rows) > 0) and np.all(keep[rows])
            E = max(1.0, np.abs(V[0, q]).max())
            nrm = np.linalg.norm(c["A"][rows], axis=1)
            assert np.all(np.abs(c["A"][rows] @ V[0, q] - c["b"][rows]) <= 1e-9 * nrm * np.maximum(E, np.abs(c["b"][rows] / nrm)))
        assert np.all(np.isnan(V[0, count[0]:])) and np.all(basis[0, count[0]:] == -1)
        results.append((V[0], count[0], status[0]))
    xh.check_cases(cases, results, "host build")


def test_degenerate_vertices_once(L, cases):
    """The reference's repeats: 12 rows for the 6 vertices of the 3-d cross-polytope, 45 .. 48 for the 8 of the 4-d one, 6 for the
    5 of the square pyramid.  The rule returns each vertex once."""
    named = [c for c in cases if c["family"] == "named"]
    want = [4, 4, 8, 6, 16, 8, 5, 8]   # cube 2, cross 2, cube 3, cross 3, cube 4, cross 4, pyramid, cube with repeats
    got = [int(xh.run(L, c["A"][None], c["b"][None])[1][0]) for c in named]
    assert got == want
    assert [len(c["R"]) for c in named][3] == 12 and len(named[5]["R"]) > 8 and len(named[6]["R"]) == 6


def test_status_and_overflow(L):
    cube = np.vstack([np.eye(3), -np.eye(3)])[None]
    one = np.ones((1, 6))
    V, count, basis, status = xh.run(L, cube, one)
    assert status[0] == xh.XS_OK and count[0] == 8
    V3, c3, b3, s3 = xh.run(L, cube, one, v_max=3)
    assert s3[0] == xh.XS_OVERFLOW and c3[0] == 3
    assert V3.tobytes() == V[:, :3].tobytes() and np.array_equal(b3, basis[:, :3])
    # exactly v_max vertices is not an overflow
    assert xh.run(L, cube, one, v_max=8)[3][0] == xh.XS_OK
    # an infeasible zero row; a harmless one; fewer live rows than dimensions; an empty intersection
    A = np.concatenate([cube, np.zeros((1, 1, 3))], axis=1)
    assert xh.run(L, A, np.r_[np.ones(6), -1.0][None])[3][0] == xh.XS_EMPTY
    V0, c0, _, s0 = xh.run(L, A, np.r_[np.ones(6), 0.0][None])
    assert s0[0] == xh.XS_OK and c0[0] == 8 and V0[:, :8].tobytes() == V.tobytes()
    assert xh.run(L, cube, one, m=np.array([2], np.int32))[3][0] == xh.XS_EMPTY
    assert xh.run(L, cube, np.r_[1.0, 1, 1, -2, 1, 1][None])[3][0] == xh.XS_EMPTY
    # a keep mask with holes: the rows that are left are the polytope
    keep = np.array([0b111111 | (1 << 7)], np.uint64)
    A = np.concatenate([cube, np.array([[[1.0, 1, 1], [1, 1, 1]]])], axis=1)
    b = np.r_[np.ones(6), 0.0, 2.0][None]    # row 6 (dropped) would cut the cube in half, row 7 cuts one corner off
    V7, c7, b7, s7 = xh.run(L, A, b, keep=keep)
    assert s7[0] == xh.XS_OK and c7[0] == 10 and set(np.unique(b7[0, :10])) == {0, 1, 2, 3, 4, 5, 7}


def test_cap_sweep_overflow_in_a_later_round(L):
    """Every cap from 1 to the full count + 1 on two members whose candidates take two rounds of 64 in the kernel: the
    12-gon's last vertex lies on rows (10, 11), subset 65 of 66; the (9, 3) polytope's last one comes from a subset of rank
    >= 64 too.  (The host build has no rounds: this pins the list the kernel is held against in tests/test_extreme_gpu.py.)"""
    (A, b), (A3, b3) = cap_sweep.extreme_members()
    V, full, basis = cap_sweep.check_extreme(A, b, lambda A, b, k: xh.run(L, A, b, v_max=k))
    assert full == 12 and basis[11].tolist() == [10, 11] and np.allclose(np.linalg.norm(V[:12], axis=1), 1.0 / np.cos(np.pi / 12))
    V, full, basis = cap_sweep.check_extreme(A3, b3, lambda A, b, k: xh.run(L, A, b, v_max=k))
    assert cap_sweep.subset_rank(basis[full - 1].tolist(), 9) >= 64 > cap_sweep.subset_rank(basis[0].tolist(), 9)


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
    prog = xh.build_program(tmp_path)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    out = subprocess.run([prog, str(path)], capture_output=True, text=True, env=env, timeout=300)
    print(out.stdout)
    assert out.returncode == 0, (out.returncode, out.stdout[-2000:], out.stderr[-4000:])
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, out.stderr[-4000:]
    assert "inconsistent: 0" in out.stdout


def test_argument_errors_need_no_library():
    from polytope_amd import batch
    A, b = np.zeros((2, 6, 3)), np.zeros((2, 6))
    for bad in (lambda: batch.extreme_batch(np.zeros((6, 3)), np.zeros(6)),
                lambda: batch.extreme_batch(A, np.zeros((2, 5))),
                lambda: batch.extreme_batch(A, np.zeros(12)),
                lambda: batch.extreme_batch(np.zeros((2, 12, 5)), np.zeros((2, 12))),
                lambda: batch.extreme_batch(np.zeros((2, 65, 3)), np.zeros((2, 65))),
                lambda: batch.extreme_batch(A, b, m=np.zeros(3, np.int32)),
                lambda: batch.extreme_batch(A, b, v_max=0),
                lambda: batch.extreme_batch(A, b, v_max=-4),
                lambda: batch.extreme_batch(A, b, v_max=2.5)):
        with pytest.raises(ValueError):
            bad()
    import polytope_amd as pa
    assert pa.extreme_batch is batch.extreme_batch
    assert [batch._extreme_vmax(d, 16) for d in (1, 2, 3, 4)] == [2, 16, 28, 104]
    assert [xh.vmax_for(d, n) for d in (1, 2, 3, 4) for n in (0, 5, 64)] == [batch._extreme_vmax(d, n) for d in (1, 2, 3, 4) for n in (0, 5, 64)]
