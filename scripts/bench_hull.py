#!/usr/bin/env python3
"""hull_batch (polytope_amd.batch, csrc/plp_hull_enum.hip: the facets of many small point sets in one launch) against the
only way to get them without it: a loop over qhull(points) with the 'hip' backend (per set a quickhull with its facet graph
on the host, then a reduce of the rows).  Both run alternately in this process -- warm-up, then >= 20 repetitions each,
every one ending in a device synchronise -- and each shape prints as one JSON line with median, minimum and maximum in ms:

  (1) 10 000 x (16 points, d = 3)      (2) 10 000 x (12, 2)      (3) 1 000 x (16, 4)

`new`: hull_batch on device-resident torch tensors with f_max given (the kernel behind its Python call; nothing is read
back); `new_sized`: f_max=None with n given as a tensor (one scalar read back).  `loop`: qhull() on the first
--loop-sets (100) point sets, scaled to the batch.  The rows of the two paths are compared once per shape on those sets.

    python scripts/bench_hull.py [--reps 20] [--warmup 3] [--rows 1,2,3] [--new-only]
Kernel times: `--new-only` under rocprofv3 --kernel-trace --stats."""
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
from polytope_amd import solvers  # noqa: E402


def stats(ts):
    return dict(median=float(np.median(ts)), min=float(np.min(ts)), max=float(np.max(ts)))


def alternate(fns, reps, warmup):
    """Every function of `fns` in turn, `reps` times, each call ending in a synchronise -> one stats dict per function."""
    for _ in range(warmup):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    ts = [[] for _ in fns]
    for _ in range(reps):
        for fn, t in zip(fns, ts):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            t.append((time.perf_counter() - t0) * 1e3)
    return [stats(t) for t in ts]


def same_rows(A, b, P):
    """The batch's rows of one set against qhull()'s polytope (reduced rows), as sets of unit-normal rows."""
    if P is None or P.A is None or not len(P.A):
        return not len(b)
    RA, Rb = np.asarray(P.A, float), np.asarray(P.b, float).ravel()
    nrm = np.linalg.norm(RA, axis=1)
    RA, Rb = RA / nrm[:, None], Rb / nrm
    if len(Rb) != len(b):
        return False
    E = max(1.0, float(np.abs(Rb).max()))
    near = (np.abs(A[:, None, :] - RA[None, :, :]).max(axis=2) + np.abs(b[:, None] - Rb[None, :]) / E) <= 1e-6
    return bool(near.any(axis=1).all() and near.any(axis=0).all())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rows", default="1,2,3")
    ap.add_argument("--loop-sets", type=int, default=100)
    ap.add_argument("--new-only", action="store_true", help="hull_batch alone (profiling runs)")
    a = ap.parse_args()
    solvers.default_solver = "hip"
    dev = torch.device("cuda:0")
    shapes = {"1": (10000, 16, 3), "2": (10000, 12, 2), "3": (1000, 16, 4)}
    for row in a.rows.split(","):
        B, n, d = shapes[row]
        X = np.random.default_rng(70 + int(row)).standard_normal((B, n, d))
        Xt = torch.as_tensor(X, device=dev)
        nt = torch.full((B,), n, dtype=torch.int32, device=dev)
        k = min(a.loop_sets, B)
        f_max = pa.batch._extreme_vmax(d, n)
        out = {}

        def new():
            out["new"] = pa.hull_batch(Xt, f_max=f_max)

        def new_sized():
            out["sized"] = pa.hull_batch(Xt, n=nt)

        def loop():
            out["loop"] = [pa.qhull(X[p].copy()) for p in range(k)]

        fns, names = [new, new_sized], ["new_ms", "new_sized_ms"]
        if not a.new_only:
            fns.append(loop)
            names.append("loop_%d_ms" % k)
        res = dict(zip(names, alternate(fns, a.reps, a.warmup)))
        line = dict(row=row, what="%d x (%d, %d)" % (B, n, d), **res)
        st = out["new"]["status"].cpu().numpy()
        cnt = out["new"]["count"].cpu().numpy()
        line["status_counts"] = {int(s): int(v) for s, v in zip(*np.unique(st, return_counts=True))}
        line["facets_mean"] = float(cnt.mean())
        line["f_max"] = int(f_max)
        if not a.new_only:
            A, b = out["new"]["A"][:k].cpu().numpy(), out["new"]["b"][:k].cpu().numpy()
            line["same_row_sets"] = int(sum(same_rows(A[p, :cnt[p]], b[p, :cnt[p]], out["loop"][p]) for p in range(k)))
            line["compared"] = k
            scaled = res["loop_%d_ms" % k]["median"] * B / k
            line["loop_scaled_to_batch_ms"] = scaled
            line["speedup_median"] = scaled / res["new_ms"]["median"]
        print(json.dumps(line))
        sys.stdout.flush()


if __name__ == "__main__":
    main()
