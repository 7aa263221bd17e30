#!/usr/bin/env python3
"""g25_convex_regions.npz -- is_convex / envelope of whole regions (2..8 members, d = 2..4) as the reference computes
them (polytope/polytope.py:988-1014, :1414-1464), for is_convex_batch / envelope_batch.

Kinds, three regions of each per dimension:
  split       a random convex polytope cut into n pieces by hyperplanes through the Chebyshev centre of its largest piece
              (convex);
  removed     the same with one of n + 1 pieces taken out (as a rule not convex);
  overlap     n random polytopes whose centres lie within half their size;
  apart       n random polytopes three sizes apart;
  nested      a random polytope and n - 1 shrunken copies inside it;
  duplicate   n - 1 overlapping polytopes, the first listed twice.

Per region every test of envelope()'s loops is run again WITHOUT the reference's skipping -- the Chebyshev radius R of
[member j; -row ii of member i] for every i, ii, j != i -- and the smallest |R - abs_tol| is recorded as `margin`.
A region is KEPT only when every R is at least 10 abs_tol above abs_tol or at most abs_tol / 10: far outside the band
(abs_tol / 2, 2 abs_tol) in which is_convex_batch hands a region to the single call, so the reference alone decides
nothing at the threshold.  (|R - abs_tol| >= 10 abs_tol cannot hold below abs_tol: a facet no partner reaches has
R = 0 and |R - abs_tol| = abs_tol, in nearly every region; below abs_tol the factor 10 is applied to R itself.)  The
script prints how many regions were dropped.

Arrays (rows as the reference's constructor leaves them; zero padding):
  d[N], n[N], kind[N] (index into `kinds`), kinds
  A[N, 8, m_max, 4], b[N, 8, m_max], m[N, 8]       the members, in list order
  convex[N]                                        is_convex(region)[0]
  env_Ab[N, e_max, 5], env_m[N]                    envelope(region) as [A | b] rows (0 rows: the empty polytope)
  margin[N]                                        min |R - abs_tol| over all tests of the region

    REF_POLYTOPE=<checkout of tulip-control/polytope> PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_convex_regions.py
"""
import os
import sys

import numpy as np

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.environ["REF_POLYTOPE"])
import polytope as pc  # noqa: E402  (the reference)

ABS_TOL = 1e-7
KINDS = ["split", "removed", "overlap", "apart", "nested", "duplicate"]
PER_KIND = 3
MAX_MEMBERS = 8


def rand_poly(rng, d, centre, size):
    """A box of half-width `size` around `centre`, cut by 1..3 random half-spaces that keep the centre."""
    k = int(rng.integers(1, 4))
    cuts = rng.standard_normal((k, d))
    cuts /= np.linalg.norm(cuts, axis=1, keepdims=True)
    A = np.vstack([np.eye(d), -np.eye(d), cuts])
    b = A @ centre + size * np.concatenate([np.ones(2 * d), rng.uniform(0.5, 0.9, k)])
    return pc.reduce(pc.Polytope(A, b))


def split(rng, P, n):
    pieces = [P]
    while len(pieces) < n:
        k = int(np.argmax([pc.cheby_ball(q)[0] for q in pieces]))
        q = pieces.pop(k)
        _, xc = pc.cheby_ball(q)
        nrm = rng.standard_normal(q.A.shape[1])
        nrm /= np.linalg.norm(nrm)
        off = float(nrm @ np.ravel(xc))
        pieces.insert(k, pc.reduce(pc.Polytope(np.vstack([q.A, nrm]), np.hstack([q.b, off]))))
        pieces.insert(k + 1, pc.reduce(pc.Polytope(np.vstack([q.A, -nrm]), np.hstack([q.b, -off]))))
    return pieces


def make(rng, kind, d, n):
    if kind == "split":
        return split(rng, rand_poly(rng, d, np.zeros(d), 1.0), n)
    if kind == "removed":
        pieces = split(rng, rand_poly(rng, d, np.zeros(d), 1.0), n + 1)
        pieces.pop(int(rng.integers(0, n + 1)))
        return pieces
    if kind == "overlap":
        return [rand_poly(rng, d, rng.uniform(-0.5, 0.5, d), float(rng.uniform(0.7, 1.0))) for _ in range(n)]
    if kind == "apart":
        return [rand_poly(rng, d, 3.0 * k * np.eye(d)[k % d] + rng.uniform(-0.2, 0.2, d), 1.0) for k in range(n)]
    if kind == "nested":
        P = rand_poly(rng, d, np.zeros(d), 1.0)
        _, xc = pc.cheby_ball(P)
        xc = np.ravel(xc)
        out = [P]
        for k in range(1, n):   # the copy scaled by s about the Chebyshev centre: A x <= s b + (1 - s) A xc
            s = 0.8 ** k
            out.append(pc.Polytope(P.A.copy(), s * P.b + (1 - s) * (P.A @ xc)))
        return out
    first = rand_poly(rng, d, np.zeros(d), 1.0)
    rest = [rand_poly(rng, d, rng.uniform(-0.5, 0.5, d), float(rng.uniform(0.7, 1.0))) for _ in range(max(n - 2, 0))]
    return [first, first.copy()] + rest


def radii(members):
    out = []
    for i, p1 in enumerate(members):
        for ii in range(p1.A.shape[0]):
            for j, p2 in enumerate(members):
                if i != j:
                    test = pc.Polytope(np.vstack([p2.A, -p1.A[ii, :]]), np.hstack([p2.b, -p1.b[ii]]))
                    out.append(float(pc.cheby_ball(test)[0]))
    return np.array(out)


def main():
    rng = np.random.default_rng(25)
    kept, dropped = [], 0
    for d in (2, 3, 4):
        for kind in KINDS:
            for _ in range(PER_KIND):
                n = int(rng.integers(2, MAX_MEMBERS + 1))
                members = make(rng, kind, d, n)
                R = radii(members)
                if np.any((R > ABS_TOL / 10) & (R < 11 * ABS_TOL)):
                    dropped += 1
                    continue
                reg = pc.Region([p.copy() for p in members])
                convex, _ = pc.is_convex(reg)
                env = pc.envelope(pc.Region([p.copy() for p in members]))
                kept.append(dict(d=d, kind=KINDS.index(kind), members=[(p.A.copy(), p.b.copy()) for p in members],
                                 convex=bool(convex), env=np.c_[env.A, env.b] if env.A.size else np.zeros((0, d + 1)),
                                 margin=float(np.abs(R - ABS_TOL).min())))
                print("d=%d %-9s n=%d rows<=%d convex=%s envelope rows=%d margin=%.3g" % (
                    d, kind, len(members), max(p.A.shape[0] for p in members), convex, kept[-1]["env"].shape[0],
                    kept[-1]["margin"]), flush=True)
    N = len(kept)
    m_max = max(a.shape[0] for r in kept for a, _ in r["members"])
    e_max = max(max(r["env"].shape[0] for r in kept), 1)
    A, b, m = np.zeros((N, MAX_MEMBERS, m_max, 4)), np.zeros((N, MAX_MEMBERS, m_max)), np.zeros((N, MAX_MEMBERS), np.int32)
    env_Ab, env_m = np.zeros((N, e_max, 5)), np.zeros(N, np.int32)
    for k, r in enumerate(kept):
        for q, (a, bb) in enumerate(r["members"]):
            m[k, q] = a.shape[0]
            A[k, q, :a.shape[0], :r["d"]], b[k, q, :a.shape[0]] = a, bb
        env_m[k] = r["env"].shape[0]
        env_Ab[k, :env_m[k], :r["d"]], env_Ab[k, :env_m[k], 4] = r["env"][:, :-1], r["env"][:, -1]
    out = os.path.join(HERE, "g25_convex_regions.npz")
    np.savez_compressed(out, d=np.array([r["d"] for r in kept], np.int32), n=np.array([len(r["members"]) for r in kept], np.int32),
                        kind=np.array([r["kind"] for r in kept], np.int32), kinds=np.array(KINDS), A=A, b=b, m=m,
                        convex=np.array([r["convex"] for r in kept]), env_Ab=env_Ab, env_m=env_m,
                        margin=np.array([r["margin"] for r in kept]))
    print("%d regions kept (%d convex), %d dropped for a radius in (abs_tol / 10, 11 abs_tol); %d bytes" % (
        N, sum(r["convex"] for r in kept), dropped, os.path.getsize(out)))


if __name__ == "__main__":
    main()
