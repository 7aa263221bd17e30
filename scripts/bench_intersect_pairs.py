#!/usr/bin/env python3
"""The overlay of two partitions -- intersect_cross_sparse (polytope_amd.batch: box cull, stacks formed on the device by
csrc/plp_pair_stack.hip, fused reduce, row emission) -- against the routes that existed before it.  Input: a C4-style grid of
box cells in d = 4 (1 000 cells, 10 x 10 x 5 x 2, and 16 000 cells, 20 x 20 x 10 x 4) and the same grid moved by half a
cell, as one table.  Routes, run alternately in this process, warm-up then --reps repetitions, every call ending in a device
synchronise, median [min - max] in ms:

    a            intersect_cross_sparse on resident tensors, at the default chunk and at --chunk
    b_total      candidates from box_pairs (resident), stacks built with numpy on the host and uploaded, reduce_batch + fm_emit
    b_resident   the same with the stacks already resident: reduce_batch + fm_emit alone (what (a) adds to is the stacking)
    c            the object loop polytope._intersect_pairs, timed ONCE on a sample of --sample candidate pairs and scaled
                 to all candidates (an estimate, printed as such)

Each size prints one JSON line.   python scripts/bench_intersect_pairs.py [--reps 20] [--warmup 3] [--sizes 1000,16000]"""
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

SHAPES = {1000: (10, 10, 5, 2), 16000: (20, 20, 10, 4)}
ABS_TOL = 1e-7


def stats(ts):
    return dict(median=float(np.median(ts)), min=float(np.min(ts)), max=float(np.max(ts)))


def alternate(fns, reps, warmup):
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


def box_cells(shape, shift):
    d = len(shape)
    idx = np.array(list(itertools.product(*[range(n) for n in shape])), dtype=float)
    n = np.array(shape, dtype=float)
    lo, hi = (idx + shift) / n, (idx + 1 + shift) / n
    A = np.tile(np.vstack([np.eye(d), -np.eye(d)])[None], (idx.shape[0], 1, 1))
    return np.ascontiguousarray(A), np.ascontiguousarray(np.concatenate([hi, -lo], 1)), lo, hi


def numpy_stacks(A, b, cand):
    """The stacks of the candidate pairs on the host: vstack, one constructor pass (no row of these cells is dropped)."""
    S = np.concatenate([A[cand[:, 0]], A[cand[:, 1]]], 1)
    h = np.concatenate([b[cand[:, 0]], b[cand[:, 1]]], 1)
    inv = 1 / np.sqrt(np.add.reduce(S * S, 2))
    return S * inv[:, :, None], h * inv


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--sizes", default="1000,16000")
    ap.add_argument("--chunk", type=int, default=8192, help="the second chunk size route (a) is timed at")
    ap.add_argument("--sample", type=int, default=200)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    pa.solvers.default_solver = "hip"
    for n in (int(s) for s in a.sizes.split(",")):
        A1, b1, lo1, hi1 = box_cells(SHAPES[n], 0.0)
        A2, b2, lo2, hi2 = box_cells(SHAPES[n], 0.5)
        A, b = np.concatenate([A1, A2]), np.concatenate([b1, b2])
        At, bt = torch.as_tensor(A, device=dev), torch.as_tensor(b, device=dev)
        lbt, ubt = torch.as_tensor(np.concatenate([lo1, lo2]), device=dev), torch.as_tensor(np.concatenate([hi1, hi2]), device=dev)
        out = {}

        def route_a():
            out["a"] = pa.intersect_cross_sparse(At, bt, n, abs_tol=ABS_TOL, boxes=(lbt, ubt))

        def route_a_chunk():
            out["a_chunk"] = pa.intersect_cross_sparse(At, bt, n, abs_tol=ABS_TOL, boxes=(lbt, ubt), chunk=a.chunk)

        def resident(St, ht):
            res = pa.reduce_batch(St, ht, abs_tol=ABS_TOL)
            live = (res["flags"] & 1) == 0
            mo = max(1, int(batch._popcount64(res["keep"][live]).max())) if bool(live.any()) else 1
            rows = batch.fm_emit(St, ht, -1, mo, keep=res["keep"], flags=res["flags"])
            return live, rows

        def route_b_total():
            cand = batch.box_pairs(lbt, ubt, n1=n)["pairs"]
            S, h = numpy_stacks(A, b, cand.cpu().numpy())
            out["St"], out["ht"] = torch.as_tensor(S, device=dev), torch.as_tensor(h, device=dev)
            out["cand"] = cand
            out["b"] = resident(out["St"], out["ht"])

        def route_b_resident():
            out["b_res"] = resident(out["St"], out["ht"])

        line = dict(n=n, grid="x".join(str(s) for s in SHAPES[n]), d=4, all_pairs=n * n, chunk=a.chunk,
                    default_chunk=batch._pair_chunk(8, 4, None))
        line["a_ms"], line["a_chunk_ms"], line["b_total_ms"], line["b_resident_ms"] = alternate(
            [route_a, route_a_chunk, route_b_total, route_b_resident], a.reps, a.warmup)
        line["reps"], line["warmup"] = a.reps, a.warmup
        line["ncand"], line["cells_out"] = int(out["a"]["ncand"]), int(out["a"]["pairs"].shape[0])
        line["stack_bytes_all_candidates"] = int(out["St"].numel() * 8 + out["ht"].numel() * 8)
        live, (rA, rb, rm) = out["b"]
        kept = out["cand"][live]
        kept[:, 1] -= n
        mo = min(int(rA.shape[1]), int(out["a"]["A"].shape[1]))
        line["routes_equal"] = bool(torch.equal(kept, out["a"]["pairs"]) and torch.equal(rm[live], out["a"]["m"])
                                    and torch.equal(rA[live][:, :mo], out["a"]["A"][:, :mo])
                                    and torch.equal(out["a"]["pairs"], out["a_chunk"]["pairs"])
                                    and torch.equal(out["a"]["A"], out["a_chunk"]["A"]))
        # (c) the object loop on a sample of the candidates, once, scaled
        cand = out["cand"].cpu().numpy()
        pick = cand[np.random.default_rng(0).choice(len(cand), size=min(a.sample, len(cand)), replace=False)]
        polys = {int(k): pa.Polytope(A[k].copy(), b[k].copy()) for k in np.unique(pick)}
        t0 = time.perf_counter()
        pa.polytope._intersect_pairs([(polys[int(i)], polys[int(j)]) for i, j in pick], ABS_TOL)
        dt = (time.perf_counter() - t0) * 1e3
        line["c_sample_ms"], line["c_sample_pairs"] = dt, int(len(pick))
        line["c_scaled_to_candidates_ms_ESTIMATE"] = dt / len(pick) * len(cand)
        print(json.dumps(line))
        sys.stdout.flush()


if __name__ == "__main__":
    main()
