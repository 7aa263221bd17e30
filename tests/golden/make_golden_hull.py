#!/usr/bin/env python3
"""g30_hull.npz -- the reference's quickhull.quickhull(points) (polytope/quickhull.py:141-359) on the families hull_batch is
held to.  Its RAW rows are recorded, not qhull()'s: qhull() passes them through reduce(), which at scale 1e-3 was seen to
drop a true facet of a 4-d hull.

Cases, in this order, from one generator default_rng(7) carried through them:
  * normal, uniform, lattice (integers in -2 .. 2: many coplanar points and exact repeats), sphere (normal points scaled to
    unit length): for each family, d in (2, 3, 4), n in (d + 1, d + 2, 8, 12, 16, 20), scale in (1, 1e-2, 1e3): the points
    times the scale, shifted by 3 scale N(0, 1);
  * cube (the 2^d corners), cube+inside (and 6 uniform points of half the size), cross (+-e_k), dup (the cube with three
    corners repeated): d in (2, 3, 4) at the three scales, shifted the same way;
  * flat: 12 normal points with the last coordinate 0 (the others scaled and shifted), d in (2, 3, 4) at the three scales.
Scales below 1e-2 are left out on purpose: the reference's abs_tol = 1e-7 is absolute.

quickhull() draws its starting simplex from numpy's global generator, which is seeded per case (seed 1000 + index).

Per case: the points, the scale, the rows quickhull() returned as they are (`A`, `b`; empty when it says "not fully
dimensional"), ref_kind (0 rows, 1 empty, 2 it raised or did not return within TIME_LIMIT seconds: on points that are
collinear to rounding its search for a starting simplex of rank d does not end), and `pinned` with a reason code.  A
case is NOT pinned when
  reason 1: two of the reference's rows (normals scaled to unit length) are between 1e-10 and 1e-7 apart in
            |dA|_inf + |db| / scale: further than its repeats of one face (which agree to rounding), closer than the distance
            at which the comparison of the tests collapses repeats -- one row to the comparison, two to an enumeration;
  reason 2: quickhull() raised or did not return.
Both rules look at the reference's output alone.  Ragged arrays are stored flat with offsets; numeric arrays and the list
of family names only.

    REF_POLYTOPE=<checkout of tulip-control/polytope> PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_hull.py
"""
import contextlib
import io
import itertools
import logging
import os
import signal
import sys
import warnings

import numpy as np

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.environ["REF_POLYTOPE"])
from polytope import quickhull as ref_quickhull  # noqa: E402  (the reference)

FAMILIES = ["normal", "uniform", "lattice", "sphere", "cube", "cube+inside", "cross", "dup", "flat"]
SCALES = (1.0, 1e-2, 1e3)
COLLAPSE, ROUNDING = 1e-7, 1e-10
TIME_LIMIT = 10   # seconds per call of quickhull(); the cases that return take milliseconds


class NoAnswer(Exception):
    pass


def _alarm(*_):
    raise NoAnswer()


def unit_rows(A, b):
    nrm = np.linalg.norm(A, axis=1)
    return A / nrm[:, None], b / nrm


def ambiguous(A, b, scale):
    if not A.size or not (np.all(np.isfinite(A)) and np.all(np.isfinite(b))):
        return False
    U, c = unit_rows(A, b)
    D = np.abs(U[:, None, :] - U[None, :, :]).max(axis=2) + np.abs(c[:, None] - c[None, :]) / scale
    return bool(np.any((D > ROUNDING) & (D <= COLLAPSE)))


def cases():
    rng = np.random.default_rng(7)
    out = []   # (family, scale, points)

    def place(P, scale):
        return P * scale + 3.0 * scale * rng.standard_normal(P.shape[1])

    for fam in ("normal", "uniform", "lattice", "sphere"):
        for d in (2, 3, 4):
            for n in (d + 1, d + 2, 8, 12, 16, 20):
                for scale in SCALES:
                    if fam == "normal":
                        P = rng.standard_normal((n, d))
                    elif fam == "uniform":
                        P = rng.uniform(-1.0, 1.0, (n, d))
                    elif fam == "lattice":
                        P = rng.integers(-2, 3, (n, d)).astype(float)
                    else:
                        P = rng.standard_normal((n, d))
                        P /= np.linalg.norm(P, axis=1)[:, None]
                    out.append((fam, scale, place(P, scale)))
    for fam in ("cube", "cube+inside", "cross", "dup"):
        for d in (2, 3, 4):
            for scale in SCALES:
                cube = np.array(list(itertools.product([-1.0, 1.0], repeat=d)))
                if fam == "cube":
                    P = cube
                elif fam == "cube+inside":
                    P = np.vstack([cube, rng.uniform(-0.5, 0.5, (6, d))])
                elif fam == "cross":
                    P = np.vstack([np.eye(d), -np.eye(d)])
                else:
                    P = np.vstack([cube, cube[[0, 1, len(cube) - 1]]])
                out.append((fam, scale, place(P, scale)))
    for d in (2, 3, 4):
        for scale in SCALES:
            P = rng.standard_normal((12, d))
            P[:, -1] = 0.0
            P = place(P, scale)
            P[:, -1] = 0.0
            out.append(("flat", scale, P))
    return out


def main():
    logging.disable(logging.CRITICAL)
    warnings.simplefilter("ignore")
    signal.signal(signal.SIGALRM, _alarm)
    fam_i, ds, scales, p_off, x_off, Xs = [], [], [], [0], [0], []
    kinds, row_off, a_off, As, bs, pinned, reason = [], [0], [0], [], [], [], []
    for index, (fam, scale, P) in enumerate(cases()):
        d = P.shape[1]
        np.random.seed(1000 + index)
        signal.alarm(TIME_LIMIT)
        try:
            with np.errstate(all="ignore"), contextlib.redirect_stdout(io.StringIO()):
                A, b, _ = ref_quickhull.quickhull(P.copy())
            A = np.array(A, dtype=float).reshape(-1, d)
            b = np.array(b, dtype=float).ravel()
            kind = 0 if len(b) else 1
        except Exception:
            A, b, kind = np.zeros((0, d)), np.zeros(0), 2
        signal.alarm(0)
        why = 2 if kind == 2 else (1 if ambiguous(A, b, scale) else 0)
        fam_i.append(FAMILIES.index(fam)); ds.append(d); scales.append(scale)
        p_off.append(p_off[-1] + P.shape[0]); x_off.append(x_off[-1] + P.size); Xs.append(P.ravel())
        kinds.append(kind); row_off.append(row_off[-1] + len(b)); a_off.append(a_off[-1] + A.size)
        As.append(A.ravel()); bs.append(b); pinned.append(why == 0); reason.append(why)
    np.savez_compressed(
        os.path.join(HERE, "g30_hull.npz"), families=np.array(FAMILIES), family=np.array(fam_i, np.int32),
        d=np.array(ds, np.int32), scale=np.array(scales), p_off=np.array(p_off, np.int64), x_off=np.array(x_off, np.int64),
        X=np.concatenate(Xs), ref_kind=np.array(kinds, np.int32), row_off=np.array(row_off, np.int64),
        a_off=np.array(a_off, np.int64), A=np.concatenate(As), b=np.concatenate(bs), pinned=np.array(pinned),
        reason=np.array(reason, np.int32))
    print("g30: %d cases, ref_kind counts %s, unpinned (index, family, reason) %s" % (
        len(kinds), np.bincount(kinds, minlength=3),
        [(i, FAMILIES[fam_i[i]], reason[i]) for i, p in enumerate(pinned) if not p]))


if __name__ == "__main__":
    main()
