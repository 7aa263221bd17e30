"""Seeded polytope families for the lane walk (polytope_amd/csrc/plp_lane_lp.hpp), shared by the host A/B test of its two
forms (tests/test_lane_walk_ab_host.py) and the GPU test of the kernels built on it (tests/test_reduce_lane_walk_gpu.py).
They are the families tests/test_lane_lp_host.py runs -- random rows, open prisms, axis-aligned boxes and cubes, ragged
row counts, rows a hair apart -- in d = 1, 2, 3."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _lattice_cuts(d):
    n = {1: [[1.0]], 2: [[1, 1], [1, -1], [-1, 1]], 3: [[1, 1, 0], [0, 1, 1], [1, 0, -1], [1, 1, 1]]}[d]
    n = np.array(n, float)
    return n / np.linalg.norm(n, axis=1)[:, None]


def families(B, d, m=16, seed=0):
    """-> list of (name, A[B, m, d], b[B, m], mrows[B] int32); rows beyond mrows[k] are zero."""
    from polytope_amd.synth import random_hpolytopes
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import soak_lane as SL
    rng = np.random.default_rng(1000 * d + seed)
    full = np.full(B, m, np.int32)
    out = []
    A, b = random_hpolytopes(B, m, d, seed=seed + d)
    out.append(("random", A, b, full))
    # ragged: random rows, no box, 1 .. m of them
    A, b = random_hpolytopes(B, m, d, seed=seed + d + 50, bounded=False)
    mr = rng.integers(1, m + 1, size=B).astype(np.int32)
    for k in range(B):
        A[k, mr[k]:] = 0.0
        b[k, mr[k]:] = 0.0
    out.append(("ragged", A, b, mr))
    # prisms: normals in a hyperplane, open along the axis left over, every other one closed on one side (unbounded box LPs)
    A = np.zeros((B, m, d))
    b = np.zeros((B, m))
    mr = np.zeros(B, np.int32)
    for k in range(B):
        Q, _ = np.linalg.qr(rng.standard_normal((d, d)))
        n = int(rng.integers(max(d, 2), 9))
        if d == 1:   # (a segment: nothing is open in R^1)
            N = np.where(np.arange(n) % 2 == 0, 1.0, -1.0)[:, None]
        else:
            G = rng.standard_normal((n, d - 1))
            G[:d - 1] = np.eye(d - 1)     # (a simplex of directions first: the cross-section is bounded)
            G[d - 1] = -1.0
            N = G @ Q[:d - 1]
            N /= np.linalg.norm(N, axis=1)[:, None]
        A[k, :n], b[k, :n] = N, 0.5 + rng.random(n)
        if k % 2 and d > 1:
            A[k, n], b[k, n] = Q[d - 1], 1.0
            n += 1
        mr[k] = n
    out.append(("prism", A, b, mr))
    # boxes with far and near cuts through corners and along edges, and bare cubes: optima on facets and edges
    box = np.vstack([np.eye(d), -np.eye(d)])
    cuts = _lattice_cuts(d)
    A = np.zeros((B, m, d))
    b = np.zeros((B, m))
    mr = np.zeros(B, np.int32)
    for k in range(B):
        lo = rng.integers(-3, 3, d) * 0.5
        hi = lo + (rng.choice([0.5, 1.0, 2.0], d) if k % 3 else 1.0)
        A[k, :2 * d], b[k, :2 * d] = box, np.r_[hi, -lo]
        n = 2 * d
        if k % 3:
            A[k, n:n + len(cuts)] = cuts
            b[k, n:n + len(cuts)] = cuts @ ((lo + hi) / 2) + rng.choice([0.2, 0.5, 5.0], len(cuts))
            n += len(cuts)
        mr[k] = n
    out.append(("box", A, b, mr))
    # dup: copies of rows, exact, with a shifted right-hand side, an ulp .. 1e-5 away
    A, b, mr = SL.make(rng, B, m, d, "dup")
    out.append(("dup", A, b, mr))
    return out
