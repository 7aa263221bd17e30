#!/usr/bin/env python3
"""g30_volume_exact.npz -- the reference's volume() (polytope/polytope.py:1529-1594) and the hull volume of its extreme()
(:1597-1682) on the families volume_exact_batch is held to.

Cases, in this order: scripts/soak_lane.py: make at the shapes (12, 2), (16, 3), (24, 3), (16, 4) -- one generator
default_rng(30) carried through the families random, ragged, dup (copies of rows 0, 1e-16 .. 1e-5 rad away), scaled, flat,
lattice with PER[family] polytopes per shape.  Ragged members with too few rows are unbounded and recorded as such.

Per case: the rows after the reference's constructor (Polytope(A, b) normalises them) and
  flat       not is_fulldim(P): its Chebyshev radius is <= 1e-7;
  unbounded  a side of its bounding_box is infinite (flat members are not looked at);
  vol_mc     volume(P, nsamples=N, seed=SEED + case) for the others, N = 10^6: the estimate is box * hits / N, so its
             standard deviation is box sqrt(p (1 - p) / N) with p = volume / box -- 1e-3 of the volume at p = 1 / 2 -- and
             `box` (the volume of the bounding box it sampled) and N are stored so that the tests recompute it;
  vol_hull   scipy.spatial.ConvexHull(extreme(P)).volume, from the first of three calls of extreme() that returned finite
             rows, NaN where none did (extreme() is not repeatable on input it has no answer for);
  extent     the largest |coordinate| of the bounding box, at least 1: the scale of the absolute part of the tolerance.
The reference alone must stay inside the cap the tests put on misses of the hull comparison (10 % of the flat family, none
elsewhere): main() checks that |vol_hull - vol_mc| <= 5 sigma wherever both exist and prints the share that does not.
Ragged arrays are stored flat with offsets; numeric arrays and the list of family names only.

    REF_POLYTOPE=<checkout of tulip-control/polytope> PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_volume_exact.py
"""
import logging
import math
import os
import sys
import warnings

import numpy as np
from scipy.spatial import ConvexHull

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.environ["REF_POLYTOPE"])
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import polytope as pc  # noqa: E402  (the reference)
import soak_lane  # noqa: E402

SHAPES = ((12, 2), (16, 3), (24, 3), (16, 4))
FAMILIES = ["random", "ragged", "dup", "scaled", "flat", "lattice"]
PER = {"random": 6, "ragged": 6, "dup": 8, "scaled": 6, "flat": 10, "lattice": 6}
N, SEED, CALLS = 1000000, 3000, 3


def cases():
    out = []   # (family, shape index, A, b)
    rng = np.random.default_rng(30)
    for fam in FAMILIES:
        for s, (m, d) in enumerate(SHAPES):
            A, b, mr = soak_lane.make(rng, PER[fam], m, d, fam)
            out += [(fam, s, A[p, :mr[p]], b[p, :mr[p]]) for p in range(PER[fam])]
    return out


def hull_volume(A, b, d):
    for _ in range(CALLS):
        try:
            with np.errstate(all="ignore"):
                R = pc.extreme(pc.Polytope(A.copy(), b.copy()))
        except Exception:
            R = None
        if R is None:
            continue
        R = np.array(R, dtype=float).reshape(-1, d)
        if not np.all(np.isfinite(R)) or len(R) < d + 1:
            continue
        try:
            return float(ConvexHull(R).volume)
        except Exception:
            continue
    return float("nan")


def main():
    logging.disable(logging.CRITICAL)
    warnings.simplefilter("ignore")
    fam_i, shape_i, ds, row_off, a_off, As, bs = [], [], [], [0], [0], [], []
    flat, unb, vol_mc, box, vol_hull, extent = [], [], [], [], [], []
    for c, (fam, s, A, b) in enumerate(cases()):
        P = pc.Polytope(A.copy(), b.copy())
        PA, Pb = np.array(P.A, dtype=float), np.array(P.b, dtype=float).ravel()
        d = PA.shape[1]
        is_flat = not pc.is_fulldim(P)
        is_unb, vm, bx, vh, ext = False, float("nan"), float("nan"), float("nan"), 1.0
        if not is_flat:
            lb, ub = P.bounding_box
            is_unb = not (np.all(np.isfinite(lb)) and np.all(np.isfinite(ub)))
            if not is_unb:
                bx = float(np.prod(ub - lb))
                ext = max(1.0, float(np.abs(lb).max()), float(np.abs(ub).max()))
                vm = float(pc.volume(P, nsamples=N, seed=SEED + c))
                vh = hull_volume(A, b, d)
        fam_i.append(FAMILIES.index(fam)); shape_i.append(s); ds.append(d)
        row_off.append(row_off[-1] + PA.shape[0]); a_off.append(a_off[-1] + PA.size); As.append(PA.ravel()); bs.append(Pb)
        flat.append(is_flat); unb.append(is_unb); vol_mc.append(vm); box.append(bx); vol_hull.append(vh); extent.append(ext)
    np.savez_compressed(
        os.path.join(HERE, "g30_volume_exact.npz"), families=np.array(FAMILIES), family=np.array(fam_i, np.int32),
        shape=np.array(shape_i, np.int32), shapes=np.array(SHAPES, np.int32), d=np.array(ds, np.int32),
        row_off=np.array(row_off, np.int64), a_off=np.array(a_off, np.int64), A=np.concatenate(As), b=np.concatenate(bs),
        flat=np.array(flat), unbounded=np.array(unb), vol_mc=np.array(vol_mc), box=np.array(box), N=np.full(len(ds), N, np.int64),
        vol_hull=np.array(vol_hull), extent=np.array(extent))
    # the reference against itself: the hull volume within 5 sigma of the estimate wherever both exist
    off, per = {}, {}
    for c in range(len(ds)):
        fam = FAMILIES[fam_i[c]]
        per[fam] = per.get(fam, 0) + 1
        if math.isfinite(vol_hull[c]) and math.isfinite(vol_mc[c]):
            p = min(max(vol_mc[c] / box[c], 0.0), 1.0)
            sg = box[c] * math.sqrt(max(p * (1 - p), 1.0 / N) / N)
            if abs(vol_hull[c] - vol_mc[c]) > 5 * sg:
                off.setdefault(fam, []).append((c, vol_hull[c], vol_mc[c], sg))
    print("g30: %d cases, %d flat, %d unbounded, %d without a hull volume; reference hull against reference estimate off by > 5 "
          "sigma: %s (of %s)" % (len(ds), sum(flat), sum(unb), sum(1 for c in range(len(ds)) if not flat[c] and not unb[c]
                                                                    and not math.isfinite(vol_hull[c])), off, per))


if __name__ == "__main__":
    main()
