#!/usr/bin/env python3
"""locate.npz -- which region holds each point, by the reference's own Region.contains / Polytope.contains
(polytope/polytope.py:206-218, :732-746), for locate_batch / Region.locate / Partition.locate.

Three sets, each a list of Regions over a domain [-1, 1]^d:
  a  d = 2: an 8 x 8 grid of box2poly cells, one single-polytope Region each (a partition);
  b  d = 3: 27 boxes, each cut by a random plane through its centre into a two-polytope Region (a partition);
  c  d = 4: 40 overlapping random polytopes, one Region each (NOT a partition: the first index matters).
Per set 2000 points are drawn uniform over 1.2 x the domain, and every point within 1e-6 |a_i| of a relaxed facet
(|a_i . x - b_i - abs_tol| for any row of any member) is dropped: only the kept points are recorded, so no comparison has
a case to excuse.

Per set S in a, b, c (rows as the reference's constructor leaves them):
  S_A[M, m_max, d], S_b[M, m_max], S_m[M]   the member polytopes, region-major, zero-padded
  S_region[M]                               the region each member belongs to
  S_X[d, N]                                 the kept points, column vectors
  S_first_region[N]                         the first region whose Region.contains holds, -1 if none
  S_first_member[N], S_count_member[N]      the first member whose Polytope.contains holds, and how many do

    REF_POLYTOPE=<checkout of tulip-control/polytope> PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_locate.py
"""
import os
import sys

import numpy as np

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.environ["REF_POLYTOPE"])
import polytope as pc  # noqa: E402  (the reference)

ABS_TOL = 1e-7
NPTS = 2000


def set_a(rng):
    e = np.linspace(-1, 1, 9)
    return [pc.Region([pc.box2poly([[e[i], e[i + 1]], [e[j], e[j + 1]]])]) for i in range(8) for j in range(8)]


def set_b(rng):
    e = np.linspace(-1, 1, 4)
    out = []
    for i in range(3):
        for j in range(3):
            for k in range(3):
                box = pc.box2poly([[e[i], e[i + 1]], [e[j], e[j + 1]], [e[k], e[k + 1]]])
                c = np.array([e[i] + e[i + 1], e[j] + e[j + 1], e[k] + e[k + 1]]) / 2
                n = rng.standard_normal(3)
                n /= np.linalg.norm(n)
                lo = pc.Polytope(np.vstack([box.A, n]), np.r_[box.b, n @ c])
                hi = pc.Polytope(np.vstack([box.A, -n]), np.r_[box.b, -(n @ c)])
                out.append(pc.Region([lo, hi]))
    return out


def set_c(rng):
    out = []
    for _ in range(40):
        c = rng.uniform(-0.8, 0.8, 4)
        R = rng.standard_normal((8, 4))
        A = np.vstack([np.eye(4), -np.eye(4), R])
        b = np.r_[c + 0.5, -(c - 0.5), R @ c + rng.uniform(0.2, 0.5, 8) * np.linalg.norm(R, axis=1)]
        out.append(pc.Region([pc.Polytope(A, b)]))
    return out


def record(name, regions, rng, out):
    members = [(r, p) for r, reg in enumerate(regions) for p in reg.list_poly]
    d = members[0][1].A.shape[1]
    m = np.array([p.A.shape[0] for _, p in members], np.int32)
    A = np.zeros((len(members), int(m.max()), d))
    b = np.zeros((len(members), int(m.max())))
    for k, (_, p) in enumerate(members):
        A[k, :m[k]], b[k, :m[k]] = p.A, np.asarray(p.b).ravel()
    X = rng.uniform(-1.2, 1.2, (d, NPTS))
    keep = np.ones(NPTS, bool)
    for _, p in members:
        gap = np.abs(p.A.dot(X) - np.asarray(p.b).ravel()[:, None] - ABS_TOL)
        keep &= np.all(gap >= 1e-6 * np.linalg.norm(p.A, axis=1)[:, None], axis=0)
    X = np.ascontiguousarray(X[:, keep])
    N = X.shape[1]
    first_region = np.full(N, -1, np.int32)
    for r in range(len(regions) - 1, -1, -1):
        first_region[regions[r].contains(X, abs_tol=ABS_TOL)] = r
    first_member = np.full(N, -1, np.int32)
    count_member = np.zeros(N, np.int32)
    for k in range(len(members) - 1, -1, -1):
        inside = members[k][1].contains(X, abs_tol=ABS_TOL)
        first_member[inside] = k
        count_member += inside
    out.update({name + "_A": A, name + "_b": b, name + "_m": m, name + "_region": np.array([r for r, _ in members], np.int32),
                name + "_X": X, name + "_first_region": first_region, name + "_first_member": first_member,
                name + "_count_member": count_member})
    print("%s: %d regions, %d members, %d of %d points kept, %d in no region, %d in more than one member" % (
        name, len(regions), len(members), N, NPTS, int((first_region < 0).sum()), int((count_member > 1).sum())))


def main():
    rng = np.random.default_rng(415)
    out = {}
    for name, make in (("a", set_a), ("b", set_b), ("c", set_c)):
        record(name, make(rng), rng, out)
    path = os.path.join(HERE, "locate.npz")
    np.savez_compressed(path, **out)
    print("%s: %d bytes" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
