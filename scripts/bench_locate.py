#!/usr/bin/env python3
"""locate_batch (polytope_amd.batch, csrc/plp_locate.hip: the first polytope containing each point) against the only device
route to the same answer without it: contains_batch(region=False), the dense uint8[P, N] matrix, and an arg-max over P.
All run alternately in this process on device-resident torch tensors -- warm-up, then >= 20 repetitions each, every one
ending in a device synchronise -- and each shape prints as one JSON line with median, minimum and maximum in ms:

  (1) the 1000-cell d = 4 partition of config C4 (10 x 10 x 5 x 2 boxes on [0, 1]^4) x 2^20 points
  (2) 10 000 x (16, 3) polytopes of synth.containment_workload x 2^20 points
  (3) 64 cells (8 x 8 boxes on [0, 1]^2) x 2^20 points

`prebuilt`: locate_batch with a LocateGrid built before the clock starts (a declined grid is the dense kernel);
`auto`: grid="auto", the grid build inside the call; `dense`: grid=None; `old`: the matrix route at N = 2^16 -- at
N = 2^20 its matrix is 1 GB at shape (1) and 10 GB at shape (2) -- and `old_scaled_ms` is that time x 16, a SCALED figure.
The answers of all routes are compared once per shape on the first 2^16 points.

--sweep: the switch point of grid="auto": P = 16 .. 4096 square cells in d = 2 x 2^20 points, dense against grid with the
build included, alternated.

    python scripts/bench_locate.py [--reps 20] [--warmup 3] [--rows 1,2,3] [--new-only] [--sweep]
Kernel times: `--new-only` under rocprofv3 --kernel-trace --stats."""
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
from polytope_amd import synth  # noqa: E402

N_FULL, N_OLD = 1 << 20, 1 << 16


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


def box_cells(shape):
    """prod(shape) boxes tiling [0, 1]^d, rows +-e_k -> A[P, 2d, d], b[P, 2d]"""
    d = len(shape)
    idx = np.array(list(itertools.product(*[range(n) for n in shape])), dtype=float)
    n = np.array(shape, dtype=float)
    A = np.tile(np.vstack([np.eye(d), -np.eye(d)])[None], (idx.shape[0], 1, 1))
    b = np.concatenate([(idx + 1) / n, -idx / n], 1)
    return np.ascontiguousarray(A), np.ascontiguousarray(b)


def workload(row):
    rng = np.random.default_rng(50 + int(row))
    if row == "1":
        A, b = box_cells((10, 10, 5, 2))
        return "1000-cell d=4 partition (C4) x 2^20 points", A, b, rng.uniform(-0.1, 1.1, (4, N_FULL))
    if row == "2":
        A, b, X = synth.containment_workload(10000, N_FULL, d=3, m=16, seed=52)
        return "10000 x (16, 3) polytopes (containment_workload) x 2^20 points", A, b, X
    A, b = box_cells((8, 8))
    return "64 cells d=2 x 2^20 points", A, b, rng.uniform(-0.1, 1.1, (2, N_FULL))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rows", default="1,2,3")
    ap.add_argument("--new-only", action="store_true", help="locate_batch alone (profiling runs)")
    ap.add_argument("--sweep", action="store_true", help="the P sweep behind the switch point of grid='auto'")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    if a.sweep:
        X = torch.as_tensor(np.random.default_rng(7).uniform(-0.1, 1.1, (2, N_FULL)), device=dev)
        for side in (4, 8, 16, 32, 64):
            A, b = box_cells((side, side))
            At, bt = torch.as_tensor(A, device=dev), torch.as_tensor(b, device=dev)
            out = {}

            def dense():
                out["d"] = pa.locate_batch(At, bt, X, grid=None)

            def grid_with_build():
                out["g"] = pa.locate_batch(At, bt, X, grid=pa.locate_grid(At, bt))

            def build_only():
                out["grid"] = pa.locate_grid(At, bt)
            res = dict(zip(["dense_ms", "grid_with_build_ms", "build_only_ms"],
                           alternate([dense, grid_with_build, build_only], a.reps, a.warmup)))
            print(json.dumps(dict(sweep_P=side * side, grid=repr(out["grid"]), equal=bool(torch.equal(out["d"], out["g"])), **res)))
            sys.stdout.flush()
        return
    for row in a.rows.split(","):
        what, A, b, X = workload(row)
        At, bt, Xt = (torch.as_tensor(np.ascontiguousarray(v), device=dev) for v in (A, b, X))
        Xs = Xt[:, :N_OLD].contiguous()
        grid = pa.locate_grid(At, bt)
        out = {}

        def prebuilt():
            out["prebuilt"] = pa.locate_batch(At, bt, Xt, grid=grid)

        def auto():
            out["auto"] = pa.locate_batch(At, bt, Xt, grid="auto")

        def dense():
            out["dense"] = pa.locate_batch(At, bt, Xt, grid=None)

        def old():
            M = pa.contains_batch(At, bt, Xs, region=False)
            out["old"] = torch.where(M.amax(0) > 0, M.argmax(0).to(torch.int32), torch.full((N_OLD,), -1, dtype=torch.int32, device=dev))
        fns, names = [prebuilt, auto, dense], ["prebuilt_ms", "auto_ms", "dense_ms"]
        if not a.new_only:
            fns.append(old)
            names.append("old_at_2^16_ms")
        res = dict(zip(names, alternate(fns, a.reps, a.warmup)))
        line = dict(row=row, what=what, P=int(A.shape[0]), N=N_FULL, grid=repr(grid), **res)
        line["routes_equal"] = bool(torch.equal(out["prebuilt"], out["dense"]) and torch.equal(out["auto"], out["dense"]))
        line["located"] = int((out["dense"] >= 0).sum())
        if not a.new_only:
            scale = N_FULL // N_OLD
            line["old_scaled_ms"] = {k: v * scale for k, v in res["old_at_2^16_ms"].items()}
            line["old_scaled_note"] = "SCALED: measured at N = 2^16, times %d" % scale
            line["old_equal_on_2^16"] = bool(torch.equal(out["old"], out["dense"][:N_OLD]))
            line["auto_median_below_old_scaled_min"] = bool(res["auto_ms"]["median"] < line["old_scaled_ms"]["min"])
        print(json.dumps(line))
        sys.stdout.flush()


if __name__ == "__main__":
    main()
