#!/usr/bin/env python3
"""g28_volume_batch.npz -- the reference's volume() (polytope/polytope.py:1529-1594) with recorded seeds, for the batched
device volume (polytope_amd.batch.volume_batch): d = 1..8, 12 and 16, 3..64 rows; random bounded polytopes, ragged row
counts, boxes, rotated boxes, thin slabs (aspect 1e3), polytopes shifted 1e3 from the origin, tiny ones (1e-3); the default
sample count and explicit ones (1, 63, 64, 65, 257, 3000, 10 000, 50 000).

Per case: the rows of the reference's Polytope (after its constructor), nsamples (-1: default), the seed, the returned
volume, the reference's bounding box and hits = round(vol / prod(ub - lb) * N).  Ragged arrays are stored flat with
offsets.

A case is kept only if every sample is at least 1e-9 away from every row (min |A x - b| >= 1e-9 on the reference's own box
and stream), so that neither the summation order of a dot product nor a 1e-9 difference in a box can flip a verdict.  The
script prints how many cases it drew again and fails if that is more than 5 % of the cases.

    REF_POLYTOPE=<checkout of tulip-control/polytope> PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_volume.py
"""
import os
import sys

import numpy as np

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.environ["REF_POLYTOPE"])
import polytope as pc  # noqa: E402  (the reference)

DIMS = [1, 2, 3, 4, 5, 6, 7, 8, 12, 16]
FAMILIES = ["random", "ragged", "box", "rotbox", "slab", "shifted", "tiny"]
EXPLICIT = [1, 63, 64, 65, 257, 3000, 10000, 50000]
MARGIN = 1e-9


def box_rows(d, half):
    return np.vstack([np.eye(d), -np.eye(d)]), np.tile(half, 2)


def rotation(rng, d):
    q, r = np.linalg.qr(rng.standard_normal((d, d)))
    return q * np.sign(np.diag(r))


def draw(rng, fam, d, full=False):
    """Rows (A, b) of a bounded polytope of family `fam` in dimension d, at most 64 rows."""
    room = 64 - 2 * d
    if fam == "box":
        lo, hi = -rng.uniform(0.5, 2.0, d), rng.uniform(0.5, 2.0, d)
        return np.vstack([np.eye(d), -np.eye(d)]), np.hstack([hi, -lo])
    if fam == "rotbox":
        A, b = box_rows(d, rng.uniform(0.5, 2.0, d))
        return A @ rotation(rng, d), b
    if fam == "slab":     # one direction 1e3 times thinner than the others
        half = rng.uniform(0.5, 2.0, d)
        half[int(rng.integers(d))] *= 1e-3
        A, b = box_rows(d, half)
        return (A @ rotation(rng, d) if d > 1 else A), b
    ncut = int(rng.integers(1, max(2, min(room, 40)) + 1)) if fam != "ragged" else int(rng.integers(1, room + 1))
    if fam == "ragged" and full:
        ncut = room      # the 64-row limit of the kernel
    elif d == 1:
        ncut = min(ncut, 6)
    C = rng.standard_normal((ncut, d))
    C /= np.linalg.norm(C, axis=1, keepdims=True)
    c = rng.uniform(0.6, 1.4, ncut) * np.sqrt(d)
    A, b = box_rows(d, np.full(d, 2.0))
    A, b = np.vstack([C, A]), np.hstack([c, b])
    if fam == "shifted":
        b = b + A @ (1e3 * rng.uniform(-1, 1, d))
    if fam == "tiny":
        b = b * 1e-3
    return A, b


def main():
    rng = np.random.default_rng(28)
    out = dict(A=[], b=[], m=[], d=[], nsamples=[], seed=[], vol=[], hits=[], lb=[], ub=[], family=[])
    redrawn, k, hist = 0, 0, []
    for fam in FAMILIES:
        for d in DIMS:
            for rep in range(3):
                # thin and tiny polytopes: a sample comes within 1e-9 of a row with a probability that grows with N m / width,
                # so the largest counts go to the families of unit size (the cap on cases drawn again decides, below)
                choices = [-1] + EXPLICIT if fam not in ("slab", "tiny") else [-1, 1, 63, 64, 65, 257, 3000, 10000]
                ns = -1 if rep == 0 else int(choices[int(rng.integers(len(choices)))])
                while True:
                    A, b = draw(rng, fam, d, full=(rep == 2))
                    if A.shape[0] < 3:   # (an interval: 3 rows at least, one of them a redundant bound)
                        A, b = np.vstack([A, A[:1]]), np.hstack([b, b[0] + 1.0])
                    P = pc.Polytope(A, b)
                    seed = int(rng.integers(0, 2 ** 62)) if rep else k
                    vol = pc.volume(P, nsamples=None if ns < 0 else ns, seed=seed)
                    l, u = P.bounding_box
                    N = ({1: 50, 2: 500, 3: 3000}.get(d, 10000)) if ns < 0 else ns
                    x = np.tile(l, (1, N)) + np.random.default_rng(seed).random((d, N)) * np.tile(u - l, (1, N))
                    res = P.A.dot(x) - P.b[:, None]
                    if np.abs(res).min() >= MARGIN and pc.is_fulldim(P):
                        break
                    redrawn += 1
                hits = int(round(vol / np.prod(u - l) * N))
                assert hits == int(np.count_nonzero(np.all(res < 0, 0))), (fam, d, rep)
                out["A"].append(P.A.ravel()); out["b"].append(P.b); out["m"].append(P.A.shape[0]); out["d"].append(d)
                out["nsamples"].append(ns); out["seed"].append(seed); out["vol"].append(vol); out["hits"].append(hits)
                out["lb"].append(l.ravel()); out["ub"].append(u.ravel()); out["family"].append(fam)
                hist.append(hits / N)
                k += 1
    n = k
    print("%d cases, %d drawn again (%.1f %%); hit fractions: %d at 0, %d at 1, median %.3f" % (
        n, redrawn, 100.0 * redrawn / n, sum(h == 0 for h in hist), sum(h == 1 for h in hist), float(np.median(hist))))
    assert redrawn <= 0.05 * n, "more than 5 % of the cases had a sample within 1e-9 of a row"
    m = np.array(out["m"], np.int64)
    d = np.array(out["d"], np.int64)
    assert m.min() >= 3 and m.max() == 64, (m.min(), m.max())
    np.savez_compressed(
        os.path.join(HERE, "g28_volume_batch.npz"), n=np.int64(n), m=m, d=d,
        A=np.concatenate(out["A"]), b=np.concatenate(out["b"]), lb=np.concatenate(out["lb"]), ub=np.concatenate(out["ub"]),
        row_off=np.concatenate([[0], np.cumsum(m)]), dim_off=np.concatenate([[0], np.cumsum(d)]),
        nsamples=np.array(out["nsamples"], np.int64), seed=np.array(out["seed"], np.int64),
        vol=np.array(out["vol"]), hits=np.array(out["hits"], np.int64), family=np.array(out["family"]))


if __name__ == "__main__":
    main()
