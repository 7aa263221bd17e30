"""CPU: the rule of envelope_batch (polytope_amd/csrc/plp_envelope.hpp built with g++ -ffp-contract=off,
tests/envelope_host.py) -- its masks against a brute force that runs every (member, row, partner) test on random regions
with the C oracle's Chebyshev radii, the stacks it asks bit for bit, the special cases (one member, 63 and 64 rows, the guard
band in both orders, a shared member, bad indices and offsets), and the stand-alone program under the sanitizers."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import envelope_host as EH  # noqa: E402
import host_build as hb  # noqa: E402

N_REGIONS = 32
ABS_TOL = 1e-7


@pytest.fixture(scope="module")
def LE(tmp_path_factory):
    return EH.build(tmp_path_factory.mktemp("envelope_host"))


def _oracle_radius(oracle):
    def radius_of(_w, _j, _ii, stack):
        return float(oracle.cheby_ball(stack[:, :-1], stack[:, -1])[0])
    return radius_of


@pytest.fixture(scope="module")
def cases(LE, oracle):
    """32 random regions, d = 1..8 in turn, 1..8 members of 1..2d + 3 rows (ragged; below d + 1 rows a member is
    unbounded): four regions of one dimension share a table, and each table runs through the rule and the brute force."""
    rng = np.random.default_rng(2025)
    radius_of = _oracle_radius(oracle)
    out = []
    for t in range(N_REGIONS // 4):
        d = t % 8 + 1
        regions = [EH.random_region(rng, d, int(rng.integers(1, 9)), 1, 2 * d + 3) for _ in range(4)]
        A, b, mc, reg_off = EH.lists_of(regions)
        got = EH.run(LE, A, b, mc, reg_off, None, ABS_TOL, radius_of)
        out.append(dict(d=d, A=A, b=b, mc=mc, reg_off=reg_off, got=got,
                        brute=EH.brute_force(A, b, mc, reg_off, None, ABS_TOL, radius_of)))
    return out


def test_rule_equals_the_brute_force(cases):
    """Test 1: equal masks and open flags, no more LPs than the brute force, and every stack asked is
    [rows of j; -row ii] bit for bit, each (w, j, ii) at most once."""
    n_regions = rule_lps = brute_lps = members = 0
    for rec in cases:
        got = rec["got"]
        outer, opened, nlp, radii = rec["brute"]
        A, b, mc, reg_off = rec["A"], rec["b"], rec["mc"], rec["reg_off"]
        assert np.array_equal(got.outer, outer), rec["d"]
        assert np.array_equal(got.status, np.where(opened, EH.ENV_OPEN, EH.ENV_OK)), rec["d"]
        assert np.all(got.nlp <= nlp) and int(got.nlp.sum()) == len(got.asked)
        seen = set()
        for w, j, ii, stack in got.asked:
            p = int(np.searchsorted(reg_off, w, side="right")) - 1
            assert (w, j, ii) in radii and (w, j, ii) not in seen
            seen.add((w, j, ii))
            assert hb.same_bits(stack, EH.stack_of(A, b, mc, int(reg_off[p]) + j, w, ii)), (w, j, ii)
        n_regions += len(reg_off) - 1
        members += len(mc)
        rule_lps += int(got.nlp.sum())
        brute_lps += int(nlp.sum())
    print("%d regions, %d members: the rule runs %d LPs, the brute force %d" % (n_regions, members, rule_lps, brute_lps))
    assert n_regions >= 24 and rule_lps < brute_lps
    assert {rec["d"] for rec in cases} == set(range(1, 9))


def _square(cx, cy, h, rows=4):
    """The square of half-width h around (cx, cy), its first `rows` rows: x <= , y <= , -x <= , -y <= ."""
    a = np.array([[1.0, 0], [0, 1.0], [-1.0, 0], [0, -1.0]])
    return a[:rows], (a @ np.array([cx, cy]) + h)[:rows]


def test_one_member_and_the_row_caps(LE):
    """Test 2a: a region of one member has every row outer and runs no LP; a member of 63 rows runs; one of 64 makes every
    entry of its list ENV_UNSUPPORTED with nothing asked, and leaves the neighbouring region alone."""
    A, b, mc, reg_off = EH.lists_of([[_square(0, 0, 1)]])
    got = EH.run(LE, A, b, mc, reg_off, None, ABS_TOL, lambda *a: 1.0)
    assert got.outer.tolist() == [15] and got.status.tolist() == [EH.ENV_OK] and got.nlp.tolist() == [0] and got.asked == []
    rng = np.random.default_rng(3)
    for rows, status in ((63, EH.ENV_OK), (64, EH.ENV_UNSUPPORTED)):
        big = EH.random_member(rng, 2, rows, np.zeros(2), 1.0)
        A, b, mc, reg_off = EH.lists_of([[big, _square(5, 5, 1)], [_square(0, 0, 1), _square(9, 9, 1)]])
        got = EH.run(LE, A, b, mc, reg_off, None, ABS_TOL, lambda *a: 0.0)
        assert got.status.tolist() == [status, status, EH.ENV_OK, EH.ENV_OK]
        if status == EH.ENV_OK:
            assert got.outer.tolist() == [(1 << 63) - 1, 15, 15, 15] and got.nlp.tolist() == [63, 4, 4, 4]
            assert [s.shape[0] for w, _, _, s in got.asked if w == 1] == [64] * 4   # (the stack of 64 rows: one per lane)
        else:
            assert got.outer.tolist() == [0, 0, 15, 15] and got.nlp.tolist() == [0, 0, 4, 4]
            assert all(w >= 2 for w, _, _, _ in got.asked)
    # a member without rows is refused too
    A, b, mc, reg_off = EH.lists_of([[_square(0, 0, 1), _square(1, 0, 1)]])
    got = EH.run(LE, A, b, np.array([4, 0], np.int32), reg_off, None, ABS_TOL, lambda *a: 1.0)
    assert got.status.tolist() == [EH.ENV_UNSUPPORTED] * 2 and got.asked == []


@pytest.mark.parametrize("unclear", [1.5e-7, 0.7e-7, float("nan")])
def test_guard_band_in_both_orders(LE, unclear):
    """Test 2b: a radius inside (abs_tol / 2, 2 abs_tol), or NaN, makes the entry ENV_OPEN only when no other partner
    crosses that row -- whether the clear partner comes before it (the unclear test is then never asked) or after it."""
    A, b, mc, reg_off = EH.lists_of([[_square(0, 0, 1), _square(1, 0, 1), _square(0, 1, 1)]])

    def radii(table):
        return lambda w, j, ii, _s: table.get((w, j, ii), 0.0)
    # entry 0, row 2: partner at position 1 unclear, nobody crosses -> open, and the row counts as outer
    got = EH.run(LE, A, b, mc, reg_off, None, ABS_TOL, radii({(0, 1, 2): unclear}))
    assert got.status.tolist() == [EH.ENV_OPEN, EH.ENV_OK, EH.ENV_OK] and got.outer.tolist() == [15, 15, 15]
    # ... the partner at position 2 crosses it clearly AFTER the unclear test
    got = EH.run(LE, A, b, mc, reg_off, None, ABS_TOL, radii({(0, 1, 2): unclear, (0, 2, 2): 0.5}))
    assert got.status.tolist() == [EH.ENV_OK] * 3 and got.outer.tolist() == [15 - 4, 15, 15]
    assert [(w, j, ii) for w, j, ii, _ in got.asked if w == 0 and ii == 2] == [(0, 1, 2), (0, 2, 2)]
    # ... the partner at position 1 crosses it clearly BEFORE: the unclear test of position 2 is not asked
    got = EH.run(LE, A, b, mc, reg_off, None, ABS_TOL, radii({(0, 1, 2): 0.5, (0, 2, 2): unclear}))
    assert got.status.tolist() == [EH.ENV_OK] * 3 and got.outer.tolist() == [15 - 4, 15, 15]
    assert [(w, j, ii) for w, j, ii, _ in got.asked if w == 0 and ii == 2] == [(0, 1, 2)]
    # at the band's ends the test has a verdict: abs_tol / 2 clears, 2 abs_tol crosses
    got = EH.run(LE, A, b, mc, reg_off, None, ABS_TOL, radii({(0, 1, 2): 0.5 * ABS_TOL, (0, 1, 3): 2 * ABS_TOL}))
    assert got.status.tolist() == [EH.ENV_OK] * 3 and got.outer.tolist() == [15 - 8, 15, 15]


def test_shared_member_bad_index_and_offsets(LE, oracle):
    """Test 2c: a member listed by two regions is tested against each region's own partners; an index outside the table
    and a decreasing reg_off make exactly the entries concerned ENV_UNSUPPORTED."""
    radius_of = _oracle_radius(oracle)
    members = [_square(0, 0, 1), _square(1, 0, 1), _square(0, 1.5, 1), _square(7, 7, 1)]
    A, b, mc = EH.pack(members)
    # region 0 = {0, 1}: the squares overlap along x; region 1 = {0, 2}: along y; region 2 = {3, 0}: apart, each
    # lies wholly beyond the two rows of the other that face it
    reg_off, mem_idx = np.array([0, 2, 4, 6], np.int32), np.array([0, 1, 0, 2, 3, 0], np.int32)
    got = EH.run(LE, A, b, mc, reg_off, mem_idx, ABS_TOL, radius_of)
    assert got.status.tolist() == [EH.ENV_OK] * 6
    assert got.outer.tolist() == [15 - 1, 15 - 4, 15 - 2, 15 - 8, 3, 12]
    want = EH.brute_force(A, b, mc, reg_off, mem_idx, ABS_TOL, radius_of)
    assert np.array_equal(got.outer, want[0]) and not want[1].any()
    # the same member twice in ONE list: each entry is the other's partner -- the twin reaches up to every row, not beyond
    got = EH.run(LE, A, b, mc, np.array([0, 2], np.int32), np.array([0, 0], np.int32), ABS_TOL, radius_of)
    assert got.outer.tolist() == [15, 15] and got.status.tolist() == [EH.ENV_OK] * 2 and got.nlp.tolist() == [4, 4]
    # an index outside the table: its whole list, and only that list
    for bad in (4, -1):
        got = EH.run(LE, A, b, mc, reg_off, np.array([0, 1, 0, bad, 3, 0], np.int32), ABS_TOL, radius_of)
        assert got.status.tolist() == [0, 0, EH.ENV_UNSUPPORTED, EH.ENV_UNSUPPORTED, 0, 0]
        assert got.outer.tolist() == [15 - 1, 15 - 4, 0, 0, 3, 12] and got.nlp[2:4].tolist() == [0, 0]
    # reg_off decreases (4 -> 3), starts above 0, or ends beyond the list: the entries no valid pair of offsets holds
    got = EH.run(LE, A, b, mc, np.array([0, 2, 4, 3], np.int32), mem_idx, ABS_TOL, radius_of)
    assert got.status.tolist() == [EH.ENV_OK] * 4 + [EH.ENV_UNSUPPORTED] * 2 and got.outer[4:].tolist() == [0, 0]
    assert all(w < 4 for w, _, _, _ in got.asked)
    got = EH.run(LE, A, b, mc, np.array([2, 2, 4, 6], np.int32), mem_idx, ABS_TOL, radius_of)
    assert got.status.tolist() == [EH.ENV_UNSUPPORTED] * 2 + [EH.ENV_OK] * 4 and got.outer[:2].tolist() == [0, 0]
    got = EH.run(LE, A, b, mc, np.array([0, 2, 4, 9], np.int32), mem_idx, ABS_TOL, radius_of)
    assert got.status.tolist() == [EH.ENV_OK] * 4 + [EH.ENV_UNSUPPORTED] * 2
    assert all(w < 4 for w, _, _, _ in got.asked)


def _write_case(f, rec, got, radii, mem_idx=None):
    A, b, mc, reg_off = rec["A"], rec["b"], rec["mc"], rec["reg_off"]
    hexs = lambda a: " ".join(float(v).hex() for v in np.ravel(a))   # noqa: E731
    n = len(got.outer)
    f.write("%d %d %d %d %d %d %s\n" % (A.shape[2], A.shape[0], A.shape[1], len(reg_off) - 1, n, mem_idx is not None,
                                         float(ABS_TOL).hex()))
    f.write(hexs(A) + "\n" + hexs(b) + "\n")
    f.write(" ".join(str(int(v)) for v in mc) + "\n" + " ".join(str(int(v)) for v in reg_off) + "\n")
    if mem_idx is not None:
        f.write(" ".join(str(int(v)) for v in mem_idx) + "\n")
    f.write("%d\n" % len(got.asked))
    for w, j, ii, _ in got.asked:
        r = radii[(w, j, ii)]
        f.write("%d %d %d %s\n" % (w, j, ii, "nan" if r != r else float(r).hex()))
    for w in range(n):
        f.write("%d %d %d\n" % (int(got.outer[w]), int(got.status[w]), int(got.nlp[w])))


def test_program_under_sanitizers(cases, LE, oracle, tmp_path):
    """Test 3: the stand-alone program runs the regions of test 1 again, the radii replayed from this run, and a list with a
    shared member and an index outside the table -- under -fsanitize=address,undefined, nothing loaded into an interpreter."""
    radius_of = _oracle_radius(oracle)
    path = os.path.join(str(tmp_path), "regions.txt")
    members = [_square(0, 0, 1), _square(1, 0, 1), _square(0, 1.5, 1)]
    A, b, mc = EH.pack(members)
    extra = dict(A=A, b=b, mc=mc, reg_off=np.array([0, 2, 4, 6], np.int32))
    idx = np.array([0, 1, 0, 2, 7, 0], np.int32)
    extra_got = EH.run(LE, A, b, mc, extra["reg_off"], idx, ABS_TOL, radius_of)
    extra_radii = {(w, j, ii): radius_of(w, j, ii, s) for w, j, ii, s in extra_got.asked}
    with open(path, "w") as f:
        f.write("%d\n" % (len(cases) + 1))
        for rec in cases:
            _write_case(f, rec, rec["got"], rec["brute"][3])
        _write_case(f, extra, extra_got, extra_radii, idx)
    prog = EH.build_program(tmp_path)
    p = subprocess.run([prog, path], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    assert "%d cases" % (len(cases) + 1) in p.stdout and "inconsistent: 0" in p.stdout, p.stdout
