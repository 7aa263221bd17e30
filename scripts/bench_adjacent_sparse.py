#!/usr/bin/env python3
"""adjacent_pairs_sparse (polytope_amd.batch: box-culled pair screen, csrc/plp_box_pairs.hip + the listed pair engines)
against the dense route to the same pairs: adjacent_pairs (all n (n - 1) / 2 stacked LPs into a uint8[n, n] matrix) and
torch.nonzero of its lower triangle.  All routes run alternately in this process on device-resident torch tensors -- warm-up,
then >= 20 repetitions each, every one ending in a device synchronise -- and each size prints as one JSON line with median,
minimum and maximum in ms.  Shapes: C4-style grids of box cells in d = 4,

    1 000 cells (10 x 10 x 5 x 2)      16 000 cells (20 x 20 x 10 x 4)      104 976 cells (18^4)

`sparse`: boxes computed inside the call (bbox_batch); `sparse_boxes`: outer boxes passed in; `dense`: the dense route, run
only while its matrix fits --dense-max-bytes (beyond: its size and LP count are printed instead, NOT a time).
`stages`: the sparse call taken apart, each stage timed on its own with a synchronise behind it -- box LPs, grid + count,
fill, pair LPs, compaction -- so their sum exceeds the call by the extra synchronises.
The pairs of all routes are compared once per size.

    python scripts/bench_adjacent_sparse.py [--reps 20] [--warmup 3] [--sizes 1000,16000,104976] [--sparse-only]
Kernel times: `--sparse-only` under rocprofv3 --kernel-trace --stats, in a run of its own."""
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
from polytope_amd import batch  # noqa: E402

SHAPES = {1000: (10, 10, 5, 2), 16000: (20, 20, 10, 4), 104976: (18, 18, 18, 18)}
ABS_TOL = 1e-7


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
    """prod(shape) boxes tiling [0, 1]^d, rows +-e_k -> A[n, 2d, d], b[n, 2d], lb[n, d], ub[n, d]"""
    d = len(shape)
    idx = np.array(list(itertools.product(*[range(n) for n in shape])), dtype=float)
    n = np.array(shape, dtype=float)
    A = np.tile(np.vstack([np.eye(d), -np.eye(d)])[None], (idx.shape[0], 1, 1))
    b = np.concatenate([(idx + 1) / n, -idx / n], 1)
    return np.ascontiguousarray(A), np.ascontiguousarray(b), idx / n, (idx + 1) / n


def stage_times(At, bt, reps, warmup):
    """The sparse call's stages, one at a time (what _pairs_sparse does in one chunk) -> {stage: stats}, candidates"""
    be = batch._Backend(At)
    n, m_max, d = (int(v) for v in At.shape)
    keep = {}

    def t_boxes():
        keep["box"] = batch._outer_boxes(be, At, bt, None, ABS_TOL)

    def t_count():
        keep["bp"] = batch._BoxPairs(be, keep["box"][0], keep["box"][1], None, batch._LOCATE_PAD, "auto")

    def t_fill():
        keep["cand"] = keep["bp"].fill()

    def t_lps():
        cand = keep["cand"]
        K = int(cand.shape[0])
        keep["v"] = be.out((K,), np.uint8)
        be.call("plp_pair_list", n, m_max, d, At, bt, None, ABS_TOL, ABS_TOL / 10, K, cand, keep["v"])

    def t_compact():
        keep["pairs"] = keep["cand"][keep["v"] != 0]
    names = ["box_lps_ms", "grid_and_count_ms", "fill_ms", "pair_lps_ms", "compaction_ms"]
    fns = [t_boxes, t_count, t_fill, t_lps, t_compact]
    res = dict(zip(names, alternate(fns, reps, warmup)))
    return res, keep


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--sizes", default="1000,16000,104976")
    ap.add_argument("--sparse-only", action="store_true", help="the sparse call alone (profiling runs)")
    ap.add_argument("--dense-max-bytes", type=float, default=float(1 << 32), help="largest n x n matrix the dense route is run for")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    for n in (int(s) for s in a.sizes.split(",")):
        A, b, lb, ub = box_cells(SHAPES[n])
        At, bt = torch.as_tensor(A, device=dev), torch.as_tensor(b, device=dev)
        boxes = (torch.as_tensor(lb - ABS_TOL, device=dev), torch.as_tensor(ub + ABS_TOL, device=dev))
        out = {}

        def sparse():
            out["sparse"] = pa.adjacent_pairs_sparse(At, bt, abs_tol=ABS_TOL)

        def sparse_boxes():
            out["sparse_boxes"] = pa.adjacent_pairs_sparse(At, bt, abs_tol=ABS_TOL, boxes=boxes)

        def dense():
            M = pa.adjacent_pairs(At, bt, abs_tol=ABS_TOL)
            out["dense"] = torch.nonzero(torch.tril(M, -1)).to(torch.int32)
        fns, names = [sparse, sparse_boxes], ["sparse_ms", "sparse_boxes_ms"]
        line = dict(n=n, grid="x".join(str(s) for s in SHAPES[n]), d=4, dense_lps=n * (n - 1) // 2, dense_matrix_bytes=n * n)
        run_dense = not a.sparse_only and n * n <= a.dense_max_bytes
        if run_dense:
            fns.append(dense)
            names.append("dense_ms")
        elif not a.sparse_only:
            line["dense_note"] = "NOT RUN: the n x n matrix (%d bytes) is beyond --dense-max-bytes; %d pair LPs" % (n * n, n * (n - 1) // 2)
        line.update(zip(names, alternate(fns, a.reps, a.warmup)))
        line["ncand"] = int(out["sparse"]["ncand"])
        line["candidates_per_cell"] = line["ncand"] / float(n)
        line["adjacent_pairs"] = int(out["sparse"]["pairs"].shape[0])
        line["boxes_routes_equal"] = bool(torch.equal(out["sparse"]["pairs"], out["sparse_boxes"]["pairs"]))
        if run_dense:
            line["dense_equal"] = bool(torch.equal(out["sparse"]["pairs"], out["dense"]))
            line["sparse_median_below_dense_min"] = bool(line["sparse_ms"]["median"] < line["dense_ms"]["min"])
        st, keep = stage_times(At, bt, a.reps, a.warmup)
        line["stages"] = st
        line["stages_equal"] = bool(torch.equal(keep["pairs"], out["sparse"]["pairs"]))
        line["grid_used"] = repr(keep["bp"].desc is not None) + " " + keep["bp"].reason
        print(json.dumps(line))
        sys.stdout.flush()


if __name__ == "__main__":
    main()
