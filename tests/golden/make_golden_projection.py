#!/usr/bin/env python3
"""g27_projection.npz -- the reference's projection() (polytope/polytope.py:1698-2114) on the families its main user
meets and on the corners of its code: random and TuLiP-shaped polytopes (a state box, an input box and `mt` target rows
pushed through x+ = Ax + Bu, projected onto the states), boxes / simplices / lattice polytopes (exact ties in the dedupe),
rows 1e-9 apart, flat and unbounded inputs, fewer rows than dimensions, solver= fm / exthull / iterhull (with a recorded
np.random.seed) / None / an unknown name, 1-D targets, and the known answers of the reference's projection_test.py.

Per case: the input (rows as passed to Polytope(A, b)), the kept coordinates (1-based), the solver, the seed, and the
output A, b, row count and status (0 a polytope, 1 Polytope(), 2 IndexError from the reference).  Ragged arrays are
stored flat with offsets.

    REF_POLYTOPE=<checkout of tulip-control/polytope> PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_projection.py
"""
import os
import sys

import numpy as np

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.environ["REF_POLYTOPE"])
import polytope as pc  # noqa: E402  (the reference)
import polytope.polytope as alg  # noqa: E402

SOLVERS = ["fm", "exthull", "iterhull", "none", "bogus", "fm_direct"]


def tulip(rng, n, k, mt):
    """A state box, an input box, and mt random target rows a.(Ax + Bu) <= c (a one-step reachability constraint)."""
    Ad = np.eye(n) + 0.2 * rng.standard_normal((n, n))
    Bd = rng.standard_normal((n, k))
    rows, rhs = [], []
    for i in range(n):
        e = np.zeros(n + k); e[i] = 1; rows += [e, -e]; rhs += [1.0 + rng.random(), 1.0 + rng.random()]
    for i in range(k):
        e = np.zeros(n + k); e[n + i] = 1; rows += [e, -e]; rhs += [1.0, 1.0]
    for _ in range(mt):
        a = rng.standard_normal(n)
        a /= np.linalg.norm(a)
        rows.append(np.hstack([a @ Ad, a @ Bd]))
        rhs.append(0.5 + rng.random())
    return np.array(rows), np.array(rhs), list(range(1, n + 1))


def random_poly(rng, d, m):
    A = rng.standard_normal((m, d))
    return A, 1.0 + rng.random(m)


def cases():
    rng = np.random.default_rng(27)
    out = []   # (kind, A, b, dim, solver, seed, tie, minrep)
    for t in range(30):   # random, 1-2 deleted dims
        d = 3 + t % 4
        A, b = random_poly(rng, d, 2 * d + t % 5)
        ndel = 1 + t % 2
        keep = sorted(rng.choice(d, d - ndel, replace=False) + 1)
        out.append(("random", A, b, keep, "fm" if t % 3 else "none", 0, False, False))
    for (n, k, mt) in ((2, 1, 6), (3, 1, 8), (3, 2, 12), (4, 2, 10)):   # TuLiP-shaped
        for t in range(5):
            A, b, dim = tulip(rng, n, k, mt)
            out.append(("tulip", A, b, dim, "fm", 0, False, False))
    for d in (3, 4, 5):   # boxes, simplices, lattice polytopes: exact ties
        box = np.vstack([np.eye(d), -np.eye(d)])
        out.append(("box", box, np.arange(1, 2 * d + 1, dtype=float), list(range(1, d)), "fm", 0, True, False))
        out.append(("box", box, np.ones(2 * d), [1, 3] if d > 3 else [1, 2], "fm", 0, True, False))
        simp = np.vstack([-np.eye(d), np.ones((1, d))])
        out.append(("simplex", simp, np.r_[np.zeros(d), 1.0], list(range(1, d)), "fm", 0, True, False))
        lat = rng.integers(-2, 3, (3 * d, d)).astype(float)
        lat = lat[np.abs(lat).sum(1) > 0]
        out.append(("lattice", lat, rng.integers(1, 4, lat.shape[0]).astype(float), list(range(1, d)), "fm", 0, True,
                    False))
        out.append(("box_minrep", box, np.ones(2 * d), list(range(2, d + 1)), "fm", 0, True, True))
    for t in range(6):   # rows a hair apart
        d = 3 + t % 3
        A, b = random_poly(rng, d, 2 * d)
        j = rng.integers(A.shape[0])
        if t % 2:
            A = np.vstack([A, A[j]]); b = np.r_[b, b[j] + 1e-9]
        else:
            A = np.vstack([A, A[j] + 1e-9 * rng.standard_normal(d)]); b = np.r_[b, b[j]]
        out.append(("hair", A, b, list(range(1, d)), "fm", 0, True, False))
    # flat and unbounded
    out.append(("flat", np.array([[1.0, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]]),
                np.array([0.0, 0, 1, 1, 1, 1]), [1, 2], "fm", 0, False, False))
    out.append(("flat", np.array([[1.0, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]]),
                np.array([1.0, 1, 1, 1, 0, 0]), [1, 2], "fm", 0, False, False))
    out.append(("unbounded", np.array([[1.0, 0, 0], [0, 1, 0], [0, 0, 1]]), np.array([1.0, 1, 1]), [1, 2], "fm", 0,
                False, False))
    out.append(("unbounded", np.array([[1.0, 1, 0], [-1, 1, 0], [0, -1, 1], [0, 0, -1]]), np.array([1.0, 1, 1, 1]),
                [1, 3], "fm", 0, False, False))
    out.append(("fewrows", np.array([[1.0, 0, 0], [0, 1, 0]]), np.array([1.0, 1]), [1, 2], "fm", 0, False, False))
    out.append(("fewrows", np.array([[1.0, 1, 1]]), np.array([1.0]), [1], None, 0, False, False))
    for t in range(8):   # solvers
        d = 3 + t % 2
        A, b = random_poly(rng, d, 3 * d)
        out.append(("exthull", A, b, [1, 2], "exthull", 0, True, False))
        out.append(("iterhull", A, b, [1, 2], "iterhull", 100 + t, True, False))
        out.append(("bogus", A, b, [2, 3], "bogus", 0, False, False))
    A, b = random_poly(rng, 5, 14)
    out.append(("auto_iterhull", A, b, [1, 2], "none", 7, True, False))
    A, b = random_poly(rng, 4, 12)
    out.append(("auto_exthull", A, b, [1], "none", 0, True, False))
    for t in range(6):   # 1-D targets
        d = 2 + t % 2
        A, b = random_poly(rng, d, 3 * d)
        out.append(("target1d", A, b, [1 + t % d], "fm", 0, False, False))
    # the reference's projection_test.py
    sq = np.array([[-1.0, 0.0], [1.0, 0.0], [0.0, -1.0], [0.0, 1.0]])
    tri = np.array([[0.0, -1.0], [1.0, 1.0], [-1.0, 1.0]])
    for A, b in ((sq, np.array([-1.0, 2.0, -1.0, 2.0])), (tri, np.array([-1.0, 4.0, 0.0]))):
        out.append(("known", A, b, [1], "fm_direct", 0, True, False))
        out.append(("known", A, b, [2], "fm_direct", 0, True, False))
    cube = np.array([[1.0, -0.0, 0.0], [-0.0, -0.0, -1.0], [-0.0, 1.0, 0.0], [1.0, 0.0, -0.0], [-0.0, -1.0, -0.0],
                     [-0.0, -0.0, 1.0], [-0.0, 0.0, -1.0], [-1.0, 0.0, 0.0], [-0.0, -1.0, 0.0], [-0.0, 1.0, -0.0],
                     [-0.0, -0.0, 1.0], [-1.0, -0.0, -0.0]])
    out.append(("known", cube, np.array([1.0, 0.0, 1.0, 1.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0, 1.0, 0.0]), [1, 2], "iterhull",
                5, True, False))
    return out


def run(pc_mod, alg_mod, A, b, dim, solver, seed, minrep):
    """(status, A_out, b_out): status 0 a polytope, 1 Polytope() (no rows), 2 IndexError."""
    P = pc_mod.Polytope(A.copy(), b.copy(), minrep=minrep)
    np.random.seed(seed)
    try:
        if solver == "fm_direct":
            d = A.shape[1]
            Q = alg_mod.projection_fm(P, None, np.setdiff1d(range(d), np.array(dim) - 1))
        else:
            Q = alg_mod.projection(P, dim, solver=None if solver == "none" else solver)
    except IndexError:
        return 2, np.zeros((0, len(dim))), np.zeros(0)
    if Q.A.size == 0:
        return 1, np.zeros((0, len(dim))), np.zeros(0)
    return 0, np.array(Q.A, dtype=float), np.array(Q.b, dtype=float).ravel()


def main():
    cs = cases()
    kinds, dims, solvers, seeds, ties, minreps = [], [], [], [], [], []
    in_d, in_off, in_A, in_b = [], [0], [], []
    dim_off, dim_v = [0], []
    out_off, out_A, out_b, status = [0], [], [], []
    for kind, A, b, dim, solver, seed, tie, minrep in cs:
        st, QA, Qb = run(pc, alg, A, b, dim, solver or "none", seed, minrep)
        kinds.append(kind); solvers.append(SOLVERS.index(solver or "none")); seeds.append(seed); ties.append(tie)
        minreps.append(minrep)
        in_d.append(A.shape[1]); in_off.append(in_off[-1] + A.shape[0]); in_A.append(A.ravel()); in_b.append(b)
        dim_v += list(dim); dim_off.append(len(dim_v))
        out_off.append(out_off[-1] + QA.shape[0]); out_A.append(QA.ravel()); out_b.append(Qb); status.append(st)
        dims.append(QA.shape[1] if QA.ndim == 2 else len(dim))
    np.savez_compressed(
        os.path.join(HERE, "g27_projection.npz"),
        kind=np.array(kinds), solver=np.array(solvers, np.int32), seed=np.array(seeds, np.int64),
        tie=np.array(ties), minrep=np.array(minreps), in_d=np.array(in_d, np.int32), in_off=np.array(in_off, np.int64),
        in_A=np.concatenate(in_A), in_b=np.concatenate(in_b), dim_off=np.array(dim_off, np.int64),
        dim=np.array(dim_v, np.int64), out_off=np.array(out_off, np.int64), out_A=np.concatenate(out_A),
        out_b=np.concatenate(out_b), out_dim=np.array(dims, np.int32), status=np.array(status, np.int32))
    print("g27: %d cases, status counts %s" % (len(cs), np.bincount(status)))


if __name__ == "__main__":
    main()
