#!/usr/bin/env python3
"""nearest_batch (polytope_amd.batch, csrc/plp_nearest.hip: K points per polytope, one dual active-set QP walk per lane)
beside support_batch at the same shape -- the yardstick: one LP walk per lane on the same tiles (the parent of the commit
that added nearest_batch has no nearest call to time).  Both run alternately in this process on device-resident torch
tensors -- warm-up, then >= 20 repetitions each, every one ending in a device synchronise -- and each shape prints as one
JSON line with median, minimum and maximum in ms:

  (1) 10 000 x (16, 3) x K = 64 points shared by all polytopes
  (2)  1 000 x (32, 4) x K = 256 points per polytope
  (3)      1 x (16, 3) x K = 2^20 points (the second grid index: K-chunks over workgroups)
  (4) the 1000-cell d = 4 grid x 2^16 points through Region.nearest (no support_batch beside it)

Beside each: the host build of the same source (tests/cabi/nearest_host.cpp) in a plain loop on one CPU core, timed on 100
problems and scaled to the shape (`cpu_scaled_ms`), and the share of problems the kernel hands back (`handback`).

    python scripts/bench_nearest.py [--reps 20] [--warmup 3] [--rows 1,2,3,4]"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402
import polytope_amd as pa  # noqa: E402
from polytope_amd import synth  # noqa: E402
from bench_support import alternate  # noqa: E402


def cpu_scaled(L, nh, A, b, X, n_total):
    """The host build on the first problems of the shape, about 100 of them, scaled to n_total -> ms."""
    B = max(1, min(A.shape[0], 100 // min(100, X.shape[-2]) or 1))
    K = min(X.shape[-2], max(1, 100 // B))
    Xs = X[:K] if X.ndim == 2 else X[:B, :K]
    t0 = time.perf_counter()
    nh.run(L, A[:B], b[:B], np.ascontiguousarray(Xs))
    return (time.perf_counter() - t0) * 1e3 * n_total / (B * K)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rows", default="1,2,3,4")
    a = ap.parse_args()
    rows = {int(r) for r in a.rows.split(",")}
    dev = torch.device("cuda:0")
    import nearest_host as nh
    L = nh.build(tempfile.mkdtemp(prefix="nearest_host_"))
    rng = np.random.default_rng(0)
    shapes = {1: (10000, 16, 3, 64, True), 2: (1000, 32, 4, 256, False), 3: (1, 16, 3, 1 << 20, True)}
    for row in sorted(rows & set(shapes)):
        B, m, d, K, shared = shapes[row]
        A, b = synth.random_hpolytopes(B, m, d, seed=row)
        X = 2.0 * rng.standard_normal((K, d) if shared else (B, K, d))
        At, bt, Xt = (torch.as_tensor(v).to(dev) for v in (A, b, X))
        xc = pa.cheby_ball_batch(At, bt)["xc"]
        raw = pa.nearest_batch(At, bt, Xt, resolve=False)
        handback = float((raw["status"] == 1).double().mean())
        new, sup = alternate([lambda: pa.nearest_batch(At, bt, Xt, resolve=False),
                              lambda: pa.support_batch(At, bt, Xt, xc=xc, resolve=False)], a.reps, a.warmup)
        print(json.dumps(dict(row=row, B=B, m=m, d=d, K=K, shared=shared, nearest_ms=new, support_ms=sup, handback=handback,
                              cpu_scaled_ms=cpu_scaled(L, nh, A, b, X, B * K))), flush=True)
    if 4 in rows:
        pa.solvers.default_solver = "hip"
        edges = [np.linspace(0.0, 1.0, n + 1) for n in (10, 10, 5, 2)]   # 10 x 10 x 5 x 2 = 1000 cells
        cells = [pa.box2poly([[edges[k][i[k]], edges[k][i[k] + 1]] for k in range(4)]) for i in np.ndindex(10, 10, 5, 2)]
        reg = pa.Region(cells)
        pts = rng.uniform(-0.5, 1.5, (4, 1 << 16))
        reg.nearest(pts[:, :64])
        (t,) = alternate([lambda: reg.nearest(pts)], a.reps, a.warmup)
        print(json.dumps(dict(row=4, cells=len(cells), d=4, N=pts.shape[1], region_nearest_ms=t)), flush=True)


if __name__ == "__main__":
    main()
