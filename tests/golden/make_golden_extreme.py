#!/usr/bin/env python3
"""g29_extreme.npz -- the reference's extreme() (polytope/polytope.py:1597-1682) on the families extreme_batch is held to.

Cases, in this order:
  * scripts/soak_lane.py: make at the shapes (17, 2), (16, 3), (24, 3), (12, 4) -- the families random, scaled, lattice with
    4 polytopes per shape from one generator default_rng(11) carried through them; then for each of the seeds 7 and 8 one
    generator carried through dup, ragged, flat, unbounded with 6 polytopes per shape;
  * the cube and the cross-polytope for d = 2, 3, 4; the square pyramid; a cube with three rows duplicated exactly and one
    redundant row.

extreme() is NOT repeatable on input it has no answer for: the same 7 rows of an unbounded polytope in d = 4 give rows
with inf in one call and finite rows of magnitude 2^56 in the next, in one process.  One call would record a roll of a
die, so every case is run CALLS = 5 times: `no_answer` counts the calls in which extreme() returned None, raised or wrote
inf / nan; `R` / `ref_kind` are those of the first call that had an answer (finite rows), or of the first call when none
had.  The tests hold a case to what the reference did: FLAT / UNBOUNDED is right only where no_answer > 0 (it did write
non-finite rows for that input), vertices are right only where some call had an answer (no_answer < CALLS), and then they
must equal R as sets.  Where the calls disagree both are accepted; in the committed file that is two cases, 186 and 191
(ragged, 7 rows in d = 4, unbounded: 2 and 3 of 5 calls without an answer).

Per case: the rows after the reference's constructor (Polytope(A, b) normalises them), what extreme() did -- ref_kind 0 it
returned rows (stored as they are, repeats and inf / nan included), 1 it returned None, 2 it raised -- and `pinned` with a
reason code.  A case is NOT pinned (reason 1) when the rows the reference returned hold two vertices that are between
1e-10 and 1e-7 of the extent E = max(1, |V|_inf) apart: further than its repeats of one degenerate vertex (which agree to
rounding, 1e-13), closer than the distance at which the comparison of the tests collapses repeats.  Such a pair -- the two
sides of a slab a few 1e-7 wide -- is two vertices to an enumeration and one to the comparison, so the case cannot be held
to equal counts.  The rule looks at the reference's output alone.
Ragged arrays are stored flat with offsets; numeric arrays and the list of family names only.

    REF_POLYTOPE=<checkout of tulip-control/polytope> PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_extreme.py
"""
import itertools
import logging
import os
import sys
import warnings

import numpy as np

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.environ["REF_POLYTOPE"])
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import polytope as pc  # noqa: E402  (the reference)
import soak_lane  # noqa: E402

SHAPES = ((17, 2), (16, 3), (24, 3), (12, 4))
FAMILIES = ["random", "scaled", "lattice", "dup", "ragged", "flat", "unbounded", "named"]
CALLS = 5   # extreme() is called this often per case (see the module text)
COLLAPSE, ROUNDING = 1e-7, 1e-10   # of the extent: the tests' collapse distance, and what repeats of one vertex stay below


def ambiguous(R):
    """Two of the reference's rows further apart than repeats of one vertex, closer than the collapse distance."""
    if not R.size or not np.all(np.isfinite(R)):
        return False
    E = max(1.0, float(np.abs(R).max()))
    D = np.abs(R[:, None, :] - R[None, :, :]).max(axis=2)
    return bool(np.any((D > ROUNDING * E) & (D <= COLLAPSE * E)))


def cases():
    out = []   # (family, A, b)
    rng = np.random.default_rng(11)
    for fam in ("random", "scaled", "lattice"):
        for (m, d) in SHAPES:
            A, b, mr = soak_lane.make(rng, 4, m, d, fam)
            out += [(fam, A[p, :mr[p]], b[p, :mr[p]]) for p in range(4)]
    for seed in (7, 8):
        rng = np.random.default_rng(seed)
        for fam in ("dup", "ragged", "flat", "unbounded"):
            for (m, d) in SHAPES:
                A, b, mr = soak_lane.make(rng, 6, m, d, fam)
                out += [(fam, A[p, :mr[p]], b[p, :mr[p]]) for p in range(6)]
    for d in (2, 3, 4):
        out.append(("named", np.vstack([np.eye(d), -np.eye(d)]), np.ones(2 * d)))
        S = np.array(list(itertools.product([-1.0, 1.0], repeat=d)))
        out.append(("named", S, np.ones(len(S))))
    out.append(("named", np.array([[0, 0, -1], [1, 0, 1], [-1, 0, 1], [0, 1, 1], [0, -1, 1]], float), np.array([0, 1, 1, 1, 1.0])))
    out.append(("named", np.vstack([np.eye(3), -np.eye(3), np.eye(3), [[1, 1, 1]]]), np.r_[np.ones(6), np.ones(3), 5.0]))
    return out


def main():
    logging.disable(logging.CRITICAL)
    warnings.simplefilter("ignore")
    fam_i, ds, row_off, a_off, As, bs = [], [], [0], [0], [], []
    kinds, ref_off, r_off, Rs, pinned, reason, no_answer = [], [0], [0], [], [], [], []
    for fam, A, b in cases():
        P = pc.Polytope(A.copy(), b.copy())
        PA, Pb = np.array(P.A, dtype=float), np.array(P.b, dtype=float).ravel()
        d = PA.shape[1]
        R, kind, lost, have_none = None, 0, 0, True
        for call in range(CALLS):
            try:
                with np.errstate(all="ignore"):
                    Rc = pc.extreme(pc.Polytope(A.copy(), b.copy()))
                kc = 1 if Rc is None else 0
            except Exception:
                Rc, kc = None, 2
            Rc = np.zeros((0, d)) if Rc is None else np.array(Rc, dtype=float).reshape(-1, d)
            gone = kc != 0 or not np.all(np.isfinite(Rc))
            lost += gone
            if call == 0 or (have_none and not gone):   # the first call, replaced by the first one that has an answer
                R, kind, have_none = Rc, kc, gone
        near = ambiguous(R)
        fam_i.append(FAMILIES.index(fam)); ds.append(d)
        row_off.append(row_off[-1] + PA.shape[0]); a_off.append(a_off[-1] + PA.size); As.append(PA.ravel()); bs.append(Pb)
        kinds.append(kind); ref_off.append(ref_off[-1] + R.shape[0]); r_off.append(r_off[-1] + R.size); Rs.append(R.ravel())
        pinned.append(not near); reason.append(1 if near else 0); no_answer.append(lost)
    np.savez_compressed(
        os.path.join(HERE, "g29_extreme.npz"), families=np.array(FAMILIES), family=np.array(fam_i, np.int32),
        d=np.array(ds, np.int32), row_off=np.array(row_off, np.int64), a_off=np.array(a_off, np.int64), A=np.concatenate(As),
        b=np.concatenate(bs), ref_kind=np.array(kinds, np.int32), ref_off=np.array(ref_off, np.int64),
        r_off=np.array(r_off, np.int64), R=np.concatenate(Rs), pinned=np.array(pinned), reason=np.array(reason, np.int32),
        calls=np.int32(CALLS), no_answer=np.array(no_answer, np.int32))
    print("g29: %d cases, ref_kind counts %s, unpinned %s, no answer in some but not all of %d calls: %s" % (
        len(kinds), np.bincount(kinds, minlength=3), [i for i, p in enumerate(pinned) if not p], CALLS,
        [(i, n) for i, n in enumerate(no_answer) if 0 < n < CALLS]))


if __name__ == "__main__":
    main()
