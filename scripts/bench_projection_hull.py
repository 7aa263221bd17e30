#!/usr/bin/env python3
"""projection_hull_batch / projection_batch(solver="iterhull") (the iterative hull of many polytopes in one launch,
polytope_amd/batch.py) on batches of horizon-shaped polytopes (polytope_amd.synth.horizon_polytopes: a state box, N input
boxes, intermediate state boxes, mt target rows through x+ = F x + G u) projected onto the states, at
(n, k, N, mt) = (2, 1, 3, 6) and (3, 1, 3, 8).  The alternatives are alternated in one process, `--reps` repetitions each,
every one ending in a device synchronise; one JSON line per shape with median [min - max] ms:
  raw       projection_hull_batch on device-resident tensors (the Chebyshev centres and the kernel)
  batch     projection_batch(solver="iterhull"): existence LP, centres, kernel, one reduce_batch, output assembly
  loop      the loop of projection(..., solver="iterhull") on 'hip', timed on `--sample` polytopes and SCALED to the batch
  fm        (first shape only) projection_batch(solver="fm")
and how many of the sampled polytopes the batch and the loop agree on (each one's vertices hold the other's rows to 1e-6
of the extent: the loop stops at 1e-7).

    python scripts/bench_projection_hull.py [--B 10000] [--reps 20] [--warmup 2] [--sample 50]
Kernel times: run the same under rocprofv3 --kernel-trace --stats."""
import argparse
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


def _stats(ms):
    return dict(median=float(np.median(ms)), min=float(np.min(ms)), max=float(np.max(ms)))


def _same_polytope(P, Q):
    VP, VQ = np.asarray(alg.extreme(P)), np.asarray(alg.extreme(Q))
    tol = 1e-6 * max(1.0, float(np.max(np.abs(VP))))
    return bool(np.max(VP @ Q.A.T - Q.b[None, :]) <= tol and np.max(VQ @ P.A.T - P.b[None, :]) <= tol)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=10000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--sample", type=int, default=50)
    ap.add_argument("--shapes", default="2,1,3,6;3,1,3,8")
    a = ap.parse_args()
    solvers.default_solver = "hip"
    dev = torch.device("cuda:0")
    for si, shp in enumerate(a.shapes.split(";")):
        n, k, N, mt = (int(v) for v in shp.split(","))
        A, b = synth.horizon_polytopes(a.B, n, k, N, mt, seed=200 + si)
        At, bt = torch.as_tensor(A, device=dev), torch.as_tensor(b, device=dev)
        dim = list(range(1, n + 1))
        idx = np.random.default_rng(si).choice(a.B, min(a.sample, a.B), replace=False)
        polys = [pa.Polytope(A[t].copy(), b[t].copy(), normalize=False) for t in idx]
        runs = {
            "raw": lambda: pa.projection_hull_batch(At, bt, dim),
            "batch": lambda: pa.projection_batch(At, bt, dim, solver="iterhull"),
            "loop": lambda: [alg.projection(p, dim, solver="iterhull") for p in polys],
        }
        if si == 0:
            runs["fm"] = lambda: pa.projection_batch(At, bt, dim, solver="fm")
        times = {key: [] for key in runs}
        last = {}
        for rep in range(a.warmup + a.reps):
            for key, fn in runs.items():
                np.random.seed(rep)   # (the loop's iterhull draws its start directions from numpy's global generator)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                last[key] = fn()
                torch.cuda.synchronize()
                if rep >= a.warmup:
                    times[key].append((time.perf_counter() - t0) * 1e3)
        res, raw = last["batch"], last["raw"]
        st = res["status"].cpu().numpy()
        Ah, bh, mh = res["A"].cpu().numpy(), res["b"].cpu().numpy(), res["m"].cpu().numpy()
        same = 0
        for j, t in enumerate(idx):
            Q = last["loop"][j]
            if Q.A.size == 0 or st[t] != 0:
                same += int(Q.A.size == 0 and st[t] == 1)
            else:
                same += int(_same_polytope(pa.Polytope(Ah[t, :mh[t]], bh[t, :mh[t]], normalize=False), Q))
        out = dict(shape=[n, k, N, mt], rows=int(A.shape[1]), d=int(A.shape[2]), B=a.B, reps=a.reps,
                   ms={key: _stats(v) for key, v in times.items()},
                   loop_scaled_ms=float(np.median(times["loop"])) * a.B / len(idx), sample=len(idx), agree=[same, len(idx)],
                   routed=int(res["routed"]), status_counts=np.bincount(st, minlength=5).tolist(),
                   kernel_status_counts=np.bincount(raw["status"].cpu().numpy(), minlength=8).tolist(),
                   lps_per_polytope=float(raw["nlp"].double().mean()), points_per_polytope=float(raw["nv"].double().mean()),
                   rows_per_projection=float(raw["m"].double().mean()))
        print(json.dumps(out))
        sys.stdout.flush()


if __name__ == "__main__":
    main()
