#!/usr/bin/env python3
"""The box pad of locate_grid (polytope_amd.batch._LOCATE_PAD), measured on the CPU: how far beyond the box of its
normalised relaxed rows can a point lie that the dense test still accepts?

Per family of scripts/soak_lane.py: make (random, ragged, unbounded, dup, scaled, flat, lattice) and shape, every polytope's
rows are relaxed and normalised as locate_grid does (batch._locate_rows), the CPU oracle boxes them (polytopes it finds
empty, flat -- Chebyshev radius < 1e-6 -- or cannot box are skipped: locate_grid lists those everywhere), and the host
restatement of the dense test (tests/locate_host.py) is run on probes where an excess can occur at all: the optimal vertex
of each of the 2d box LPs pushed outwards along its axis by 1e-17 .. 1e-5 of max(1, |bound|), and uniform points in the box
blown up by the same factors.  Reported: the worst excess of an accepted probe beyond the box, relative to max(1, |bound|),
per family; the pad is max(1e-9, 1000 x the worst).  One JSON line per family, one for the total.

    python scripts/measure_locate_pad.py [polytopes per family and shape, default 40]"""
import json
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

import soak_lane  # noqa: E402
import locate_host as LH  # noqa: E402
from oracle import oracle as O  # noqa: E402
from polytope_amd import batch as pb  # noqa: E402

FAMILIES = ["random", "ragged", "unbounded", "dup", "scaled", "flat", "lattice"]
SHAPES = ((12, 2), (16, 3), (16, 4))
DELTAS = 10.0 ** np.arange(-17.0, -4.5, 0.5)
TOL = 1e-7


def main():
    per = int(sys.argv[1]) if len(sys.argv) > 1 else 40
    O.build()
    L = LH.build(tempfile.mkdtemp())
    rng = np.random.default_rng(415)
    total = dict(worst=0.0, accepted_outside=0, probes=0, boxed=0, skipped=0)
    for fam in FAMILIES:
        worst, outside, probes, boxed, skipped = 0.0, 0, 0, 0, 0
        for m_rows, d in SHAPES:
            A, b, m = soak_lane.make(rng, per, m_rows, d, fam)
            An, bn, every, nowhere = pb._locate_rows(LH._Numpy(), A, b, m, TOL)
            lb, ub, status = LH.oracle_boxes(O, An, bn, m)
            for p in range(per):
                if status[p] or every[p] or nowhere[p]:
                    skipped += 1
                    continue
                boxed += 1
                mp = int(m[p])
                X = []
                for k in range(d):
                    for sign, bound in ((1.0, ub[p, k]), (-1.0, lb[p, k])):
                        if not np.isfinite(bound):
                            continue
                        c = np.zeros(d)
                        c[k] = -sign
                        st, x, _, _ = O.lp_solve(c, An[p, :mp], bn[p, :mp])
                        if st != 0:
                            continue
                        for dl in DELTAS:
                            y = x.copy()
                            y[k] = bound + sign * dl * max(1.0, abs(bound))
                            X.append(y)
                fin = np.isfinite(lb[p]) & np.isfinite(ub[p])
                cen, half = np.where(fin, (lb[p] + ub[p]) / 2, 0.0), np.where(fin, (ub[p] - lb[p]) / 2, 1.0)
                for dl in DELTAS[::4]:
                    U = cen[None] + (1 + dl) * half[None] * rng.uniform(-1, 1, (200, d))
                    X.extend(U)
                X = np.ascontiguousarray(np.array(X).T)
                first, _ = LH.locate(L, A[p:p + 1, :mp], b[p:p + 1, :mp], X, TOL)
                acc = X[:, first == 0]
                probes += X.shape[1]
                with np.errstate(invalid="ignore"):
                    ex = np.maximum((acc - ub[p][:, None]) / np.maximum(1.0, np.abs(ub[p]))[:, None],
                                    (lb[p][:, None] - acc) / np.maximum(1.0, np.abs(lb[p]))[:, None])
                ex = np.where(np.isfinite(ex), ex, -np.inf).max(0) if acc.shape[1] else np.zeros(0)
                outside += int((ex > 0).sum())
                worst = max(worst, float(ex.max()) if ex.size else 0.0)
        print(json.dumps(dict(family=fam, worst_relative_excess=worst, accepted_outside_box=outside, probes=probes,
                              polytopes_boxed=boxed, polytopes_skipped=skipped)))
        total["worst"] = max(total["worst"], worst)
        total["accepted_outside"] += outside
        total["probes"] += probes
        total["boxed"] += boxed
        total["skipped"] += skipped
    total["pad"] = max(1e-9, 1000 * total["worst"])
    total["pad_in_use"] = pb._LOCATE_PAD
    print(json.dumps(total))


if __name__ == "__main__":
    main()
