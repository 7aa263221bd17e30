#!/usr/bin/env python3
"""g31_projection_hull.npz -- the reference's projection(p, dim, solver="iterhull") (polytope/polytope.py:1955-2100) on the
families projection_hull_batch is held to.  The generator runs the reference on the CPU; it imports it and copies none of it.

Cases, in this order, from one generator default_rng(31) carried through them (the horizon shapes: polytope_amd.synth):
  * random   m random unit rows tangent to spheres of radius 0.5 .. 0.9 plus the 2 d rows of the box |x| <= 1:
             (m, d) -> k = (16, 5) -> 2, (20, 6) -> 2, (14, 5) -> 3, (28, 8) -> 2, five of each, onto the first k coordinates;
  * horizon  synth.horizon_polytopes at (n, k, N, mt) = (2, 1, 3, 6), (2, 2, 2, 6), (3, 1, 3, 8), (3, 2, 3, 8), five of each,
             onto the states;
  * box      axis boxes in R^5 and R^6 onto 2 and 3 coordinates, and prisms (a box times a simplex): every LP is degenerate
             and many vertices project to one point;
  * triangle the triangle (0, 0), (1, 1), (0.5, 0.2), whose four box points are collinear, lifted to d = 4 by |x_3|, |x_4| <= 1;
  * open     unbounded along a deleted coordinate only (the projection is bounded: PH_OK), and unbounded along a kept
             one (PH_UNBOUNDED; the reference is not asked: its iterhull has no answer there);
  * identity d = k = 2 and 3: a random polytope onto all of its coordinates;
  * line     k = 1 at d = 3, 5 and 8;
  * overflow random (24, 8) -> 3 (24 random rows at radius 0.3 .. 0.6 and the 16 of the box), two of them: more than 64
             vertices,
             PH_OVERFLOW_POINTS.

The reference's iterhull draws directions from numpy's global generator, which is seeded per case (seed 3100 + index).

Per case: the rows as the reference's Polytope holds them (`A`, `b`), `dim` (1-based), `expect` (the status the rule must
give), the rows of the reference's projection (`ref_A`, `ref_b`), extreme() of it (`ref_V`), ref_kind (0 rows, 1 it
returned Polytope(), 2 it raised, 3 not asked), ref_gap -- the largest amount by which the support value of the INPUT
polytope in a reference row's direction (unit length) exceeds that row's right-hand side, the support LPs by the oracle's
certified LP, never below 0 -- and `pinned` with a reason code.  A case is NOT pinned when
  reason 1: two of the reference's rows (unit normals) are between 1e-10 and 1e-7 apart in |dA|_inf + |db| / scale;
  reason 2: the reference raised, or returned Polytope() for a projection onto two or more coordinates that exists (onto
            one coordinate it always does: its qhull() takes no two points on a line; those cases stay pinned -- their
            expected status does not come from the reference -- and check (c) has nothing to compare);
  reason 3: ref_gap exceeds 1e-6 scale (the reference stopped short of its own 1e-7 by more than ten times).
All three look at the reference's output alone.  Ragged arrays are stored flat with offsets.

    REF_POLYTOPE=<checkout of tulip-control/polytope> PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_projhull.py
"""
import contextlib
import io
import logging
import os
import sys
import warnings

import numpy as np

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.environ["REF_POLYTOPE"])
import polytope as ref  # noqa: E402  (the reference)
sys.path.insert(0, ROOT)
from oracle import oracle  # noqa: E402
from polytope_amd import synth  # noqa: E402

FAMILIES = ["random", "horizon", "box", "triangle", "open", "identity", "line", "overflow"]
COLLAPSE, ROUNDING, GAP_LIMIT = 1e-7, 1e-10, 1e-6
PH_OK, PH_UNBOUNDED, PH_OVERFLOW_POINTS = 0, 1, 3


def random_rows(rng, m, d, lo=0.5, hi=0.9):
    """m random unit rows tangent to spheres of radius lo .. hi, and the 2 d rows of the box |x| <= 1 in front of them."""
    A = rng.standard_normal((m, d))
    A /= np.linalg.norm(A, axis=1)[:, None]
    return np.vstack([np.eye(d), -np.eye(d), A]), np.concatenate([np.ones(2 * d), rng.uniform(lo, hi, m)])


def box_rows(lo, hi):
    d = len(lo)
    return np.vstack([np.eye(d), -np.eye(d)]), np.concatenate([hi, -np.asarray(lo)])


def cases():
    rng = np.random.default_rng(31)
    out = []   # (family, A, b, dim, expect, ask the reference)
    for (m, d, k) in ((16, 5, 2), (20, 6, 2), (14, 5, 3), (28, 8, 2)):
        for _ in range(5):
            A, b = random_rows(rng, m, d)
            out.append(("random", A, b, np.arange(1, k + 1), PH_OK, True))
    for (n, k, N, mt) in ((2, 1, 3, 6), (2, 2, 2, 6), (3, 1, 3, 8), (3, 2, 3, 8)):
        A, b = synth.horizon_polytopes(5, n, k, N, mt, seed=31, stream=len(out))
        for i in range(5):
            out.append(("horizon", A[i], b[i], np.arange(1, n + 1), PH_OK, True))
    for (d, dim) in ((5, (1, 2)), (5, (2, 4, 5)), (6, (1, 6)), (6, (1, 3, 5))):
        lo = rng.uniform(-2.0, -0.5, d)
        hi = rng.uniform(0.5, 2.0, d)
        A, b = box_rows(lo, hi)
        out.append(("box", A, b, np.array(dim), PH_OK, True))
    for (d, dim) in ((5, (1, 2)), (5, (1, 2, 3)), (6, (2, 3, 4))):
        # a prism: the box, cut by sum of the first three coordinates <= 1
        A, b = box_rows(-np.ones(d), np.ones(d))
        cut = np.zeros(d)
        cut[:3] = 1.0
        out.append(("box", np.vstack([A, cut]), np.concatenate([b, [1.0]]), np.array(dim), PH_OK, True))
    # the triangle (0, 0), (1, 1), (0.5, 0.2) in (x_1, x_2): rows through its edges, inward side by the third vertex
    T = np.array([[0.0, 0.0], [1.0, 1.0], [0.5, 0.2]])
    rows, rhs = [], []
    for i in range(3):
        p, q, r = T[i], T[(i + 1) % 3], T[(i + 2) % 3]
        nrm = np.array([q[1] - p[1], p[0] - q[0]])
        if nrm @ (r - p) > 0:
            nrm = -nrm
        rows.append(np.concatenate([nrm, [0.0, 0.0]]))
        rhs.append(nrm @ p)
    A, b = box_rows([-1.0, -1.0], [1.0, 1.0])
    A4 = np.hstack([np.zeros((4, 2)), A])
    out.append(("triangle", np.vstack([np.array(rows), A4]), np.concatenate([rhs, b]), np.array([1, 2]), PH_OK, True))
    # open along the deleted x_5 only / along the kept x_1
    A, b = random_rows(rng, 16, 5)
    A5 = A.copy()
    A5[:, 4] = np.where(A5[:, 4] > 0, 0.0, A5[:, 4])   # nothing bounds x_5 from above (the constructor drops the zero row)
    out.append(("open", A5, b, np.array([1, 2]), PH_OK, True))
    A, b = random_rows(rng, 16, 5)
    A1 = A.copy()
    A1[:, 0] = np.where(A1[:, 0] > 0, 0.0, A1[:, 0])
    live = np.linalg.norm(A1, axis=1) > 0
    out.append(("open", A1[live], b[live], np.array([1, 2]), PH_UNBOUNDED, False))
    for d in (2, 3):
        A, b = random_rows(rng, 2 * d, d)
        out.append(("identity", A, b, np.arange(1, d + 1), PH_OK, True))
    for (m, d, j) in ((8, 3, 2), (14, 5, 5), (20, 8, 1)):
        A, b = random_rows(rng, m, d)
        out.append(("line", A, b, np.array([j]), PH_OK, True))
    for _ in range(2):
        A, b = random_rows(rng, 24, 8, 0.3, 0.6)
        out.append(("overflow", A, b, np.array([1, 2, 3]), PH_OVERFLOW_POINTS, True))
    return out


def ambiguous(A, b, scale):
    U, c = A / np.linalg.norm(A, axis=1)[:, None], b / np.linalg.norm(A, axis=1)
    D = np.abs(U[:, None, :] - U[None, :, :]).max(axis=2) + np.abs(c[:, None] - c[None, :]) / scale
    return bool(np.any((D > ROUNDING) & (D <= COLLAPSE)))


def main():
    logging.disable(logging.CRITICAL)
    warnings.simplefilter("ignore")
    cols = {key: [] for key in ("family", "d", "m", "k", "A", "b", "dim", "expect", "ref_kind", "ref_A", "ref_b", "ref_V",
                                "ref_gap", "pinned", "reason", "nvert")}
    for index, (fam, A, b, dim, expect, ask) in enumerate(cases()):
        p = ref.Polytope(A, b)
        A, b = np.array(p.A, dtype=float), np.array(p.b, dtype=float)
        d, k = A.shape[1], len(dim)
        rA, rb, rV, kind, gap, why = np.zeros((0, k)), np.zeros(0), np.zeros((0, k)), 3, 0.0, 0
        if ask:
            np.random.seed(3100 + index)
            try:
                with np.errstate(all="ignore"), contextlib.redirect_stdout(io.StringIO()):
                    q = ref.projection(ref.Polytope(A.copy(), b.copy()), list(dim), solver="iterhull")
                    rA, rb = np.array(q.A, dtype=float).reshape(-1, k), np.array(q.b, dtype=float).ravel()
                    kind = 0 if rb.size else 1
                    if kind == 0:
                        rV = np.array(ref.extreme(q), dtype=float).reshape(-1, k)
            except Exception:
                rA, rb, rV, kind = np.zeros((0, k)), np.zeros(0), np.zeros((0, k)), 2
            if kind == 0:
                scale = float(np.max((rV.max(axis=0) - rV.min(axis=0)) / 2.0))
                for a, bb in zip(rA, rb):
                    c = np.zeros(d)
                    c[dim - 1] = a / np.linalg.norm(a)
                    st, _, fun, _ = oracle.lp_solve(-c, A, b)
                    assert st == 0, (index, st)
                    gap = max(gap, -fun - bb / np.linalg.norm(a))
                why = 1 if ambiguous(rA, rb, scale) else (3 if gap > GAP_LIMIT * scale else 0)
            else:
                why = 2 if (kind == 2 or k > 1) else 0
            assert kind != 0 or (rV.shape[0] > 64) == (expect == PH_OVERFLOW_POINTS), (index, fam, rV.shape[0])
        cols["family"].append(FAMILIES.index(fam)); cols["d"].append(d); cols["m"].append(A.shape[0]); cols["k"].append(k)
        cols["A"].append(A.ravel()); cols["b"].append(b); cols["dim"].append(np.asarray(dim, dtype=np.int32))
        cols["expect"].append(expect); cols["ref_kind"].append(kind); cols["ref_A"].append(rA.ravel()); cols["ref_b"].append(rb)
        cols["ref_V"].append(rV.ravel()); cols["ref_gap"].append(gap); cols["pinned"].append(why == 0); cols["reason"].append(why)
        cols["nvert"].append(rV.shape[0])

    def off(key):
        return np.concatenate([[0], np.cumsum([len(v) for v in cols[key]])]).astype(np.int64)
    np.savez_compressed(
        os.path.join(HERE, "g31_projection_hull.npz"), families=np.array(FAMILIES), family=np.array(cols["family"], np.int32),
        d=np.array(cols["d"], np.int32), m=np.array(cols["m"], np.int32), k=np.array(cols["k"], np.int32),
        a_off=off("A"), A=np.concatenate(cols["A"]), b_off=off("b"), b=np.concatenate(cols["b"]),
        dim_off=off("dim"), dim=np.concatenate(cols["dim"]), expect=np.array(cols["expect"], np.int32),
        ref_kind=np.array(cols["ref_kind"], np.int32), ra_off=off("ref_A"), ref_A=np.concatenate(cols["ref_A"]),
        rb_off=off("ref_b"), ref_b=np.concatenate(cols["ref_b"]), rv_off=off("ref_V"), ref_V=np.concatenate(cols["ref_V"]),
        ref_gap=np.array(cols["ref_gap"]), pinned=np.array(cols["pinned"]), reason=np.array(cols["reason"], np.int32))
    print("g31: %d cases, ref_kind counts %s, vertices %s, worst ref_gap %.3g, unpinned (index, family, reason) %s" % (
        len(cols["d"]), np.bincount(cols["ref_kind"], minlength=4), cols["nvert"], max(cols["ref_gap"]),
        [(i, FAMILIES[cols["family"][i]], cols["reason"][i]) for i, ok in enumerate(cols["pinned"]) if not ok]))


if __name__ == "__main__":
    main()
