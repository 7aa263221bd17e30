#!/usr/bin/env python3
"""The device volume (polytope_amd.batch.volume_batch, csrc/plp_volume.hip) against the sample-upload path it replaces
(polytope._volume_by_samples: samples drawn by numpy on the host, uploaded, containment kernel, bytes back).  Both paths
run alternately in this process -- warm-up, then >= 20 repetitions each, every one ending in a device synchronise -- and
each row prints as one JSON line with the median, minimum and maximum of both in ms:

  (a) volume(Region): a 1000-cell d = 4 grid of boxes; 10 000 random (16, 3) polytopes
  (b) volume(Polytope) at d = 2 / 3 / 4 with the default sample count
  (c) volume_batch alone on device-resident arrays: 10 000 x (16, 3) x 3000, 10 000 x (32, 4) x 10 000, 1 x (16, 3) x 10^7;
      the old path here is the per-polytope loop on a sample of the batch, extrapolated (10^7: the one call itself)
  (d) is_subset(200 cells, 1000 cells) and Region(1000 cells).intersect(P) with volume() as it is and with the old loop

    python scripts/bench_volume.py [--reps 20] [--warmup 3] [--rows a,b,c,d] [--new-only]
Kernel times and counters: `--rows c --new-only` under rocprofv3 --kernel-trace --stats, and under --pmc in runs of their own."""
import argparse
import itertools
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402
import polytope_amd as pa  # noqa: E402
from polytope_amd import solvers, synth  # noqa: E402
from polytope_amd import polytope as alg  # noqa: E402


def old_volume(polyreg, nsamples=None, seed=None):
    """volume() as it was before the device path: a Python loop of sample uploads over the members of a Region."""
    if not alg.is_fulldim(polyreg):
        return 0.0
    if isinstance(polyreg, alg.Region):
        alg.bounding_box(polyreg)
        tot = 0.0
        for p in polyreg.list_poly:
            tot += old_volume(p)
        polyreg._set_volume(tot)
        return tot
    return alg._volume_by_samples(polyreg, nsamples, seed)


NEW_ONLY = False


def stats(ts):
    return dict(median=float(np.median(ts)), min=float(np.min(ts)), max=float(np.max(ts)))


def alternate(new, old, reps, warmup, old_scale=1.0):
    if NEW_ONLY:   # (profiling runs: only the new path's kernels in the trace)
        old = lambda: None  # noqa: E731
    for _ in range(warmup):
        new()
        old()
    torch.cuda.synchronize()
    tn, to = [], []
    for _ in range(reps):
        for fn, ts in ((new, tn), (old, to)):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
    return stats(tn), stats(np.array(to) * old_scale)


def report(row, what, new, old, **extra):
    print(json.dumps(dict(row=row, what=what, new_ms=new, old_ms=old, speedup_median=old["median"] / new["median"], **extra)))
    sys.stdout.flush()


def grid_cells(shape):
    d = len(shape)
    return [pa.box2poly([[i[k] / shape[k], (i[k] + 1) / shape[k]] for k in range(d)])
            for i in itertools.product(*[range(n) for n in shape])]


def random_polys(B, m, d, seed):
    A, b = synth.random_hpolytopes(B, m, d, seed=seed, bounded=True)
    return [pa.Polytope(A[k], b[k]) for k in range(B)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rows", default="a,b,c,d")
    ap.add_argument("--new-only", action="store_true", help="skip the old path (its columns are then meaningless)")
    a = ap.parse_args()
    global NEW_ONLY
    NEW_ONLY = a.new_only
    rows = a.rows.split(",")
    solvers.default_solver = "hip"
    dev = torch.device("cuda:0")
    if "a" in rows:
        for what, polys in (("volume(Region of a 10x10x5x2 grid of boxes, d=4)", grid_cells((10, 10, 5, 2))),
                            ("volume(Region of 10000 random (16, 3) polytopes)", random_polys(10000, 16, 3, 11))):
            R = alg.Region(polys)
            alg.volume(R)   # boxes, balls and the resident table: cached for both paths
            new, old = alternate(lambda: alg.volume(R), lambda: old_volume(R), a.reps, a.warmup)
            report("a", what, new, old, members=len(polys))
    if "b" in rows:
        for d in (2, 3, 4):
            P = random_polys(1, 16, d, 20 + d)[0]
            alg.volume(P)
            new, old = alternate(lambda: alg.volume(P), lambda: alg._volume_by_samples(P), a.reps, a.warmup)
            report("b", "volume(Polytope (16, %d)), default nsamples" % d, new, old)
    if "c" in rows:
        for B, m, d, N, sample in ((10000, 16, 3, 3000, 200), (10000, 32, 4, 10000, 100), (1, 16, 3, 10 ** 7, 1)):
            A, b = synth.random_hpolytopes(B, m, d, seed=30 + d, bounded=True)
            polys = [pa.Polytope(A[k], b[k], normalize=False) for k in range(min(B, sample))]
            At, bt = torch.as_tensor(A, device=dev), torch.as_tensor(b, device=dev)
            box = pa.bbox_batch(At, bt)
            for p in polys:
                p.bounding_box
            res = {}

            def new():
                res["r"] = pa.volume_batch(At, bt, nsamples=N, seed=7, lb=box["lb"], ub=box["ub"])

            def old():
                for p in polys:
                    alg._volume_by_samples(p, N, 7)
            tn, to = alternate(new, old, a.reps, a.warmup, old_scale=B / len(polys))
            hits = int(res["r"]["hits"].sum())
            report("c", "volume_batch %d x (%d, %d) x %d" % (B, m, d, N), tn, to, old_is_extrapolated_from=len(polys),
                   hits_total=hits, gsamples_per_s=B * N / tn["median"] / 1e6)
    if "d" in rows:
        cells = grid_cells((10, 10, 5, 2))
        A, b = synth.random_hpolytopes(1, 12, 4, seed=4, bounded=True)
        P = pa.Polytope(A[0], 0.1 * b[0] + A[0] @ (0.5 * np.ones(4)))
        flows = (("is_subset(200 cells, 1000 cells)",
                  lambda: pa.is_subset(pa.Region([c.copy() for c in cells[:200]]), pa.Region([c.copy() for c in cells]))),
                 ("Region(1000 cells).intersect(P)", lambda: pa.Region([c.copy() for c in cells]).intersect(P.copy())))
        current = alg.volume
        for what, fn in flows:
            def old():
                alg.volume = old_volume
                try:
                    fn()
                finally:
                    alg.volume = current
            new, old_t = alternate(fn, old, a.reps, a.warmup)
            report("d", what, new, old_t)


if __name__ == "__main__":
    main()
