"""CPU: the library's region_diff search (polytope_amd/csrc/plp_rdiff_search.hpp built with g++ -ffp-contract=off,
tests/rdiff_host.py) against its Python twin polytope._DiffSearch, piece for piece, on the random overlapping boxes of
the GPU parity test; that speculation, small sub-batches and an emptied memo never change the pieces; the odd turns of
the reference's INDICES arithmetic on hand-made tables; and the stand-alone program under the sanitizers."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import rdiff_host as RH  # noqa: E402

N_TRIALS = 24


@pytest.fixture(scope="module")
def L(tmp_path_factory):
    return RH.build(tmp_path_factory.mktemp("rdiff_host"))


class SharedRadii(object):
    """The radius function both searches read: region_diff's own `radii_rows` behind ONE dict keyed by the row tuple
    (indices below zero wrapped as numpy wraps them), NaN = no verdict kept as it comes.  The LPs go to the C oracle on
    the rows as the Polytope constructor normalises them (pcm._radii replaced while `radii_rows` runs): 0 for a ball
    solved with r < 0, NaN for any status but 0 -- the reading of polytope._radii(nan_without_verdict=True)."""

    def __init__(self, radii_rows, nrows, oracle):
        self.radii_rows, self.nrows, self.oracle, self.known = radii_rows, nrows, oracle, {}

    def _radii(self, polys, nan_without_verdict=False):
        out = []
        for p in polys:
            if p.A.ndim != 2 or p.A.shape[0] == 0:
                out.append(float("nan") if nan_without_verdict else 0)
                continue
            st, r, _ = self.oracle.cheby(p.A, p.b)
            out.append((float("nan") if nan_without_verdict else 0) if st != 0 else (0 if r < 0 else r))
        return out

    def key(self, rows):
        k = tuple(int(r) + self.nrows if r < 0 else int(r) for r in rows)
        if any(not 0 <= r < self.nrows for r in k):
            raise IndexError("row index out of range")
        return k

    def __call__(self, row_lists):
        import polytope_amd.polytope as pcm
        keys = [self.key(r) for r in row_lists]
        new = [k for k in dict.fromkeys(keys) if k not in self.known]
        if new:
            saved, pcm._radii = pcm._radii, self._radii
            try:
                for k, r in zip(new, self.radii_rows([list(k) for k in new])):
                    self.known[k] = r
            finally:
                pcm._radii = saved
        return [self.known[k] for k in keys]


@pytest.fixture(scope="module")
def searches(L, oracle):
    """region_diff on the scipy backend over the 24 random cases, with polytope._DiffSearch replaced by a wrapper that
    runs the real twin AND the host-built search on the same table, tolerance and radii -> one record per search."""
    import polytope_amd.polytope as pcm
    from polytope_amd import solvers
    records = []
    real = pcm._DiffSearch
    reopen = real._reopen_after_piece

    class Both(object):
        def __init__(self, m, mi, beg, M, abs_tol, radii_rows, look_ahead):
            self.rec = dict(m=int(m), mi=[int(v) for v in mi], tol=abs_tol,
                            radii=SharedRadii(radii_rows, int(m) + 2 * int(M), oracle), twin_asked=set(), reopened=set())
            rec = self.rec

            def spy(row_lists):
                tw = self.twin
                if tw.level != -1 and tw.counter[tw.level] == 0:   # a scan: the node re-opened if no cell hits
                    rows = list(tw.rows)
                    try:
                        if not reopen(tw, list(tw.counter), rows, tw.level)[1]:
                            rec["reopened"].add(rec["radii"].key(rows))
                    except IndexError:
                        pass
                out = rec["radii"](row_lists)
                rec["twin_asked"].update(rec["radii"].key(r) for r in row_lists)
                return out
            self.twin = real(m, mi, beg, M, abs_tol, spy, look_ahead)

        def run(self):
            rec = self.rec
            rec["wrapped"] = 0

            def spy(twin, counter, rows, level):   # "level - 1" reaches -1 with open cells left: the LAST cell is read
                rec["wrapped"] += level - 1 == -1 and any(c != 0 for c in counter)
                return reopen(twin, counter, rows, level)
            real._reopen_after_piece = spy
            try:
                rec["twin"] = [(kind, rec["radii"].key(rows)) for kind, rows in self.twin.run()]
            except IndexError:
                rec["twin"] = "IndexError"
            finally:
                real._reopen_after_piece = reopen
            rec["host"] = RH.search(L, rec["m"], rec["mi"], rec["tol"], rec["radii"])
            records.append(rec)
            if rec["twin"] == "IndexError":
                raise IndexError("region_diff twin")
            for kind, rows in rec["twin"]:
                yield kind, list(rows)

    saved_solver, solvers.default_solver = solvers.default_solver, "scipy"
    pcm._DiffSearch = Both
    try:
        for trial, (P, cells) in enumerate(RH.random_cases(N_TRIALS)):
            n0 = len(records)
            try:
                pcm.region_diff(P.copy(), pcm.Region([c.copy() for c in cells]))
            except IndexError:
                pass
            for rec in records[n0:]:
                rec["trial"] = trial
    finally:
        pcm._DiffSearch = real
        solvers.default_solver = saved_solver
    return records


def test_twin_piece_for_piece(searches):
    """Case 1: the same (kind, rows) sequence as the twin, or "row index out of range" exactly where the twin raises."""
    assert sorted(rec["trial"] for rec in searches) == list(range(N_TRIALS))   # every case reached its search, once
    compared = 0
    for rec in searches:
        twin, host = rec["twin"], rec["host"]
        print("trial %d: %s pieces, host code %d, %d lists asked, level -1 with open cells %d times" % (
            rec["trial"], twin if twin == "IndexError" else len(twin), host.code, len(host.asked), rec["wrapped"]))
        if twin == "IndexError":
            assert host.code == RH.BAD_INDEX, rec["trial"]
            continue
        assert host.code == RH.OK, (rec["trial"], host.code)
        assert host.leaves == twin, rec["trial"]
        compared += 1
    assert compared >= 20


def test_speculation_never_changes_the_result(L, searches):
    """Case 2, first 9 cases: default knobs against all five knobs at 0 -- identical leaves and n_requests.  With all
    knobs 0 the search asks every list the twin reads and, as the search always did, two kinds of list no knob turns
    off: the scan lists of a missed node (read when the node is not empty) and the one node re-opened after a piece
    (read when the scan hits no cell); nothing else."""
    for rec in searches:
        if rec["trial"] >= 9 or rec["twin"] == "IndexError":
            continue
        m, mi = rec["m"], rec["mi"]
        beg = m + np.concatenate([[0], np.cumsum(mi[:-1])]).astype(int)
        full = rec["host"]
        bare = RH.search(L, m, mi, rec["tol"], rec["radii"], knobs=RH.NO_SPECULATION)
        assert bare.code == full.code == RH.OK
        assert bare.leaves == full.leaves and bare.n_requests == full.n_requests, rec["trial"]
        assert full.leaves == RH.search(L, m, mi, rec["tol"], rec["radii"], knobs=RH.DEFAULT_KNOBS).leaves
        asked = bare.asked
        assert len(asked) == len(set(asked)) and rec["twin_asked"] <= set(asked), rec["trial"]
        assert len(asked) < len(full.asked)
        blocks = [tuple(range(beg[j], beg[j] + mi[j])) for j in range(len(mi))]
        extra = 0
        for batch in bare.batches:
            for k, w in enumerate(batch):
                if w in rec["twin_asked"] or any(w[-len(b):] == b for b in blocks):
                    continue
                # neither read by the twin nor a scan list: the node re-opened after a piece, queued last with a scan
                assert k == len(batch) - 1 and w in rec["reopened"], (rec["trial"], w)
                extra += 1
        print("trial %d: %d lists without speculation, %d re-opened nodes the twin never reads" % (rec["trial"], len(asked), extra))


def _table_radii(radius_of, cap=5000):
    known, calls = {}, [0]

    def radii(row_lists):
        calls[0] += 1   # (radii that no polytope has can send the walk round in circles: end it)
        assert calls[0] < cap, "the search does not end on this table"
        for w in row_lists:
            if w not in known:
                known[w] = radius_of(w)
        return [known[w] for w in row_lists]
    return radii


def _twin(m, mi, tol, radii):
    import polytope_amd.polytope as pcm
    mi = [int(v) for v in mi]
    M = sum(mi)
    beg = [m + sum(mi[:j]) for j in range(len(mi))]
    nrows = m + 2 * M

    def checked(row_lists):
        keys = [tuple(r + nrows if r < 0 else r for r in w) for w in row_lists]
        if any(not 0 <= r < nrows for w in keys for r in w):
            raise IndexError("row index out of range")
        return radii(keys)
    try:
        return [(k, tuple(r + nrows if r < 0 else r for r in rows))
                for k, rows in pcm._DiffSearch(m, mi, beg, M, tol, checked, look_ahead=False).run()]
    except IndexError:
        return "IndexError"


def _interval_radius(m, mi, lo0, hi0, cells):
    """d = 1: rows 0..1 = x <= hi0, -x <= -lo0; cell j: x <= hi_j, -x <= -lo_j; then the negations."""
    rows = [(1, hi0), (-1, -lo0)] + [r for lo, hi in cells for r in ((1, hi), (-1, -lo))]
    rows += [(-s, -b) for s, b in rows[2:]]

    def radius(w):
        ub = min([rows[r][1] for r in w if rows[r][0] > 0] or [np.inf])
        lb = max([-rows[r][1] for r in w if rows[r][0] < 0] or [-np.inf])
        return float("nan") if not np.isfinite(ub - lb) else max(0.0, 0.5 * (ub - lb))
    return radius


ODD_TABLES = {
    # one cell whose two rows both cut the minuend: [0, 1] minus [0.3, 0.6]
    "one_cell": (2, [2], _interval_radius(2, [2], 0.0, 1.0, [(0.3, 0.6)])),
    # the last cell closes with an earlier one still open: "level - 1" walks on
    "two_cells": (2, [2, 2], _interval_radius(2, [2, 2], 0.0, 1.0, [(0.2, 0.5), (0.4, 0.8)])),
    "three_cells": (2, [2, 2, 2], _interval_radius(2, [2, 2, 2], 0.0, 1.0, [(0.1, 0.3), (0.25, 0.6), (0.5, 0.9)])),
    # every list full-dimensional, whatever its rows: the walk visits every sign pattern
    "always_full": (1, [1, 2, 1], lambda w: 1.0),
    "always_full_two_cells": (2, [2, 1], lambda w: 1.0),
    # nothing is ever full-dimensional: the first scan ends the search with the minuend as the only piece
    "never_full": (2, [1, 1], lambda w: 0.0),
    # no LP ever gives a verdict
    "all_nan": (2, [2, 1], lambda w: float("nan")),
    # full-dimensional by a hash of the list: pieces and empty nodes alternate in no geometric order
    "hash": (2, [3, 1, 2, 2], lambda w: 1.0 if (sum((i + 1) * r for i, r in enumerate(w)) % 5) in (0, 2, 3) else 0.0),
    "hash7": (1, [1, 1, 1, 1, 1], lambda w: 1.0 if (sum((i + 2) * (r + 1) for i, r in enumerate(w)) % 7) in (1, 2, 4, 6) else 0.0),
}


@pytest.mark.parametrize("name", sorted(ODD_TABLES))
def test_odd_turns(L, name):
    """Case 3: hand-made tables -- intervals, and radii no polytope has (always / never full-dimensional, no verdict
    anywhere, a hash of the list) -- on which the host-built search ends exactly as the twin does, whatever is
    speculated.  All of them end with pieces; the turns no whole search takes are in test_moves_on_hand_made_states."""
    m, mi, radius_of = ODD_TABLES[name]
    radii = _table_radii(radius_of)
    want = _twin(m, mi, 1e-7, radii)
    for knobs in (None, RH.NO_SPECULATION, (600, 3, 12, 1, 1)):
        got = RH.search(L, m, mi, 1e-7, radii, knobs=knobs)
        if want == "IndexError":
            assert got.code == RH.BAD_INDEX, knobs
        else:
            assert got.code == RH.OK and got.leaves == want, knobs


def _twin_move(m, mi, counter, idx, level, which):
    """the twin's move on an explicit state -> what RH.move returns, or "IndexError" where the twin's own indexing raises"""
    import polytope_amd.polytope as pcm
    mi = [int(v) for v in mi]
    M = sum(mi)
    nrows = m + 2 * M
    tw = pcm._DiffSearch(m, mi, [m + sum(mi[:j]) for j in range(len(mi))], M, 1e-7, None, False)
    counter, rows = list(counter), list(idx)
    try:
        level, ended = (tw._next_sibling if which == 0 else tw._reopen_after_piece)(counter, rows, level)
    except IndexError:
        return "IndexError"
    ok = all(-nrows <= v < nrows for v in rows)   # what numpy's indexing of the table accepts
    return level, ended, counter, rows, sum(counter), [v + nrows if v < 0 else v for v in rows] if ok else None


MOVE_STATES = [
    # (m, mi, counter, idx, level, move): level 0 with an open cell, the LAST cell's counter above mi -- "level - 1" reads
    # the last cell through Python's negative index, closes it and ends the search at level == -1
    (2, [2, 1], [1, 2], [0, 1, 5, 7], 0, 1),
    (2, [2, 2, 1], [1, 0, 3], [0, 1, 7, 11], 0, 1),
    # ... the last cell's counter within mi: it is re-opened at level -1, and the search goes on from there
    (2, [2, 1], [1, 1], [0, 1, 5, 7], 0, 1),
    (2, [2, 2], [2, 0], [0, 1, 2, 7], 0, 1),
    # a counter above mi one level down: closed, then the same level is looked at again with the counter at 0
    (2, [1, 2], [3, 1], [0, 1, 5, 6], 1, 1),
    # "- M" on a row of the minuend: the index wraps to the end of the table / leaves it
    (2, [2, 1], [1, 0], [0, 1], 1, 1),
    (1, [3, 3], [1, 1], [-9], 1, 1),
    (1, [3, 3], [2, 0], [0, -12], 0, 0),
    (2, [1], [0], [0, 1, 99], 0, 0),
    (2, [2, 2], [1, 2], [0, 1, 6, 9], 1, 0),
    # next_sibling through two exhausted cells down to level -1
    (2, [1, 1], [1, 1], [0, 1, 4, 5], 1, 0),
    (2, [1, 2, 1], [0, 2, 1], [0, 1, 3, 8], 2, 0),
]
# an EMPTY list of indices and an open cell whose counter is within mi: "- M" on the last index has nothing to act on.
# The twin's `rows[-1] -= M` raises IndexError; both C++ states note it and their resolve fails (BAD_INDEX / RD_INDEX).
# m = 0 and m >= 1, next_sibling and reopen_after_piece (the last one re-opens the LAST cell at level -1)
EMPTY_LIST_STATES = [
    (0, [2], [1], [], 0, 0),
    (0, [2, 1], [1, 0], [], 1, 1),
    (2, [2], [1], [], 0, 0),
    (1, [1, 2], [0, 1], [], 0, 1),
]
MOVE_STATES += EMPTY_LIST_STATES
# ... and an empty list that no move reads: the one open cell is exhausted, closed, and the search ends
MOVE_STATES.append((0, [1], [2], [], 0, 0))


def test_moves_on_hand_made_states(L):
    """Case 3, the turns no whole search takes.  A piece is emitted only by a scan that hit no cell; that scan runs at a
    level whose counter is 0, and every open cell lies below it (next_sibling closes a cell before the walk leaves it
    downwards, a hit opens the cell the level moves to) -- so at level 0 no cell is open, and "level - 1" reaches -1
    with nothing to re-open: the 24 random cases and the tables above never get there with an open cell, nor did a
    search over small tables with made-up radii find an index out of range.  The moves take an explicit state on both
    sides, so they are compared directly: hand-made states at level 0 with open cells and a counter above mi, indices
    that wrap or leave the table, an empty list of indices, and 3 000 random states; plp::rdiff::State under the moves
    of plp_rdiff_walk.hpp against the twin's _next_sibling / _reopen_after_piece, field for field, and resolve against
    numpy's reading of the indices (where the twin's own indexing raises IndexError, resolve must fail)."""
    rng = np.random.default_rng(5)
    states = list(MOVE_STATES)
    for _ in range(3000):
        N = int(rng.integers(1, 5))
        m = int(rng.integers(1, 4))
        mi = [int(v) for v in rng.integers(1, 4, N)]
        nrows = m + 2 * sum(mi)
        counter = [int(rng.integers(0, mi[j] + 3)) if rng.random() < 0.6 else 0 for j in range(N)]
        idx = [int(v) for v in rng.integers(-nrows - 4 if rng.random() < 0.3 else 0, nrows + (4 if rng.random() < 0.2 else 0),
                                            int(rng.integers(1, m + sum(counter) + 3)))]
        states.append((m, mi, counter, idx, int(rng.integers(0, N)), int(rng.integers(0, 2))))
    seen = dict(ended_at_minus_one_with_open_cells=0, reopened_at_minus_one=0, out_of_range=0, wrapped=0, trimmed=0)
    for m, mi, counter, idx, level, which in states:
        want = _twin_move(m, mi, counter, idx, level, which)
        got = RH.move(L, m, mi, counter, idx, level, which)
        if want == "IndexError":   # the twin's own indexing raised: the State's resolve must fail
            assert got[5] is None, (m, mi, counter, idx, level, which)
            continue
        assert got == want, (m, mi, counter, idx, level, which)
        lvl, ended, _, rows_after, _, table_rows = got
        if which == 1 and level == 0 and any(counter):
            seen["ended_at_minus_one_with_open_cells" if ended else "reopened_at_minus_one"] += 1
        seen["out_of_range"] += table_rows is None
        seen["wrapped"] += table_rows is not None and any(v < 0 for v in rows_after)
        seen["trimmed"] += len(rows_after) < len(idx)
    print(seen)
    assert all(v >= 5 for v in seen.values()), seen
    for st in EMPTY_LIST_STATES:
        assert _twin_move(*st) == "IndexError" and RH.move(L, *st)[5] is None
    assert RH.move(L, *MOVE_STATES[-1]) == (-1, True, [0], [], 0, [])
    for st in MOVE_STATES[:2]:
        assert RH.move(L, *st)[:2] == (-1, True)
    assert [RH.move(L, *st)[5] is None for st in MOVE_STATES[5:10]] == [False, True, True, True, False]


def test_small_batches_and_an_emptied_memo(L, searches):
    """Case 4: a backend that takes 3 lists / 64 rows at a time cuts every scan into several sub-batches, and a memo of
    400 entries is emptied again and again (a list is asked a second time only after that): the same leaves."""
    emptied = cut = 0
    for rec in searches:
        if rec["trial"] >= 9 or rec["twin"] == "IndexError":
            continue
        full = rec["host"]
        got = RH.search(L, rec["m"], rec["mi"], rec["tol"], rec["radii"], cap_lp=3, cap_rows=64, memo_limit=400)
        assert got.code == RH.OK and got.leaves == full.leaves and got.n_requests == full.n_requests, rec["trial"]
        assert max(len(b) for b in got.batches) <= 3 and max(sum(len(w) for w in b) for b in got.batches) <= 64
        cut += len(got.batches) > len(full.batches)
        emptied += len(got.asked) > len(set(got.asked))
        assert len(full.asked) == len(set(full.asked))   # (the default memo is never emptied at this size)
    assert cut >= 3 and emptied >= 3
    # a list longer than a sub-batch holds ends the search with its own code
    rec = searches[0]
    assert RH.search(L, rec["m"], rec["mi"], rec["tol"], rec["radii"], cap_rows=rec["m"]).code == RH.LIST_TOO_LONG


def test_program_under_sanitizers(tmp_path):
    """Case 5: the stand-alone program (axis-aligned tables, closed-form radii) under -fsanitize=address,undefined."""
    prog = RH.build_program(tmp_path)
    p = subprocess.run([prog], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    assert "inconsistent: 0" in p.stdout, p.stdout
