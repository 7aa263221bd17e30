#!/usr/bin/env python3
"""region_diff_search_batch (polytope_amd.batch, csrc/plp_rdiff_batch.hip: many region_diff searches in one launch, one per
wavefront) against the only way to run them without it: a loop of batch.region_diff_search calls (per search a table
upload, a resident LP server and a host round trip per visited node).  Both run alternately in this process -- warm-up,
then >= 20 repetitions each, every one ending in a device synchronise -- and each shape prints as one JSON line with
median, minimum and maximum in ms:

  (1) 10 000 x (minuend (9, 3), 4 box cells each)      (2) 1 000 x ((12, 4), 8 box cells each)
  (3) 200 members of the 1000-cell d = 4 grid of config C4 (10 x 10 x 5 x 2 boxes on [0, 1]^4), each moved by half a cell
      along every axis, against the grid cells it overlaps (up to 16)

What region_diff does in front of the search (unit rows, the radii of the stacks in one cheby_ball_batch, the cells that do
not intersect dropped, the rest ordered) is done once, outside the timing, for both sides.  `new`: the batch on
device-resident torch tensors with p_max / r_max given (nothing is read back); `new_numpy`: the same from numpy arrays
with the wrapper's own sizing (upload, status read back, a second launch for the problems that overflowed).  `loop`:
region_diff_search on the first --loop-problems (100) problems that have a cell left, on the tables the batch built, scaled
to the batch.  The leaves of the two are compared on those problems.

    python scripts/bench_region_diff_batch.py [--reps 20] [--warmup 3] [--rows 1,2,3] [--new-only]
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
from polytope_amd import batch, solvers  # noqa: E402


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


def boxes(lo, hi):
    """lo, hi [n, d] -> rows x <= hi, -x <= -lo of n boxes: A[n, 2d, d], b[n, 2d]."""
    n, d = lo.shape
    A = np.broadcast_to(np.concatenate([np.eye(d), -np.eye(d)])[None], (n, 2 * d, d)).copy()
    return A, np.concatenate([hi, -lo], axis=1)


def random_problems(B, m, d, n_cells, seed):
    """B minuends of m random unit rows around (0.5, ..) as in the parity tests, n_cells overlapping boxes each."""
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((B, m, d))
    A /= np.linalg.norm(A, axis=2)[:, :, None]
    b = 0.3 * (1 + rng.random((B, m))) + A @ (0.5 * np.ones(d))
    cen, hw = rng.random((B * n_cells, d)), rng.uniform(0.05, 0.3, (B * n_cells, d))
    CA, Cb = boxes(cen - hw, cen + hw)
    return A, b, CA, Cb, np.arange(0, B * n_cells + 1, n_cells), np.arange(B * n_cells)


def grid_problems(n_members):
    shape = np.array([10, 10, 5, 2])
    w = 1.0 / shape
    ijk = np.stack(np.unravel_index(np.arange(int(shape.prod())), shape), axis=1)
    CA, Cb = boxes(ijk * w, (ijk + 1) * w)
    pick = np.random.default_rng(4).choice(len(ijk), n_members, replace=False)
    lo, hi = (ijk[pick] + 0.5) * w, (ijk[pick] + 1.5) * w
    A, b = boxes(lo, hi)
    off, idx = [0], []
    for k in range(n_members):   # the cells whose interior meets the moved member
        touch = np.all((ijk * w < hi[k] - 1e-12) & ((ijk + 1) * w > lo[k] + 1e-12), axis=1)
        idx.extend(np.nonzero(touch)[0])
        off.append(len(idx))
    return A, b, CA, Cb, np.asarray(off), np.asarray(idx)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rows", default="1,2,3")
    ap.add_argument("--loop-problems", type=int, default=100)
    ap.add_argument("--new-only", action="store_true", help="the batch alone (profiling runs)")
    a = ap.parse_args()
    solvers.default_solver = "hip"
    dev = torch.device("cuda:0")
    makers = {"1": ("10000 x ((9, 3), 4 cells)", lambda: random_problems(10000, 9, 3, 4, 71)),
              "2": ("1000 x ((12, 4), 8 cells)", lambda: random_problems(1000, 12, 4, 8, 72)),
              "3": ("200 moved members of the C4 grid x the cells they overlap", lambda: grid_problems(200))}
    for row in a.rows.split(","):
        what, make = makers[row]
        A, b, CA, Cb, off, idx = make()
        pre = batch._rdiff_prepare(A, b, None, CA, Cb, None, off, idx, 1e-7, None)
        args = [pre[k] for k in ("A", "b", "m", "CA", "Cb", "mc", "cell_off", "cell_idx")]
        sized = batch.region_diff_search_batch(*args)   # (also the sizes the device-resident call is given)
        p_max, r_max = max(1, int(sized["count"].max())), max(1, int(sized["nrows"].max()))
        targs = [torch.as_tensor(x, device=dev) for x in args]
        B, d = A.shape[0], A.shape[2]
        out = {}

        def new():
            out["new"] = batch.region_diff_search_batch(*targs, p_max=p_max, r_max=r_max)

        def new_numpy():
            out["numpy"] = batch.region_diff_search_batch(*args)

        # the tables the loop runs on: the minuend's rows, the new rows by `src`, their negations
        flatA, flatb = pre["CA"].reshape(-1, d), pre["Cb"].ravel()
        todo = [p for p in range(B) if sized["status"][p] == batch.RD_OK and pre["cell_off"][p + 1] > pre["cell_off"][p]]
        todo = todo[:a.loop_problems]
        tables = []
        for p in todo:
            m, N = int(pre["m"][p]), int(pre["cell_off"][p + 1] - pre["cell_off"][p])
            mi = sized["mi"][p][:N]
            src = sized["src"][p][:int(mi.sum())]
            TA = np.concatenate([pre["A"][p, :m], flatA[src], -flatA[src]])
            Tb = np.concatenate([pre["b"][p, :m], flatb[src], -flatb[src]])
            tables.append((TA, Tb, m, mi))

        def loop():
            out["loop"] = [batch.region_diff_search(*t) for t in tables]

        fns, names = [new, new_numpy], ["new_ms", "new_numpy_ms"]
        if not a.new_only:
            fns.append(loop)
            names.append("loop_%d_ms" % len(todo))
        res = dict(zip(names, alternate(fns, a.reps, a.warmup)))
        line = dict(row=row, what=what, **res)
        st = out["new"]["status"].cpu().numpy()
        line["status_counts"] = {int(s): int(v) for s, v in zip(*np.unique(st, return_counts=True))}
        line["lps"] = int(sized["nlp"].sum())
        line["pieces"] = int(sized["count"].sum())
        line["p_max"], line["r_max"] = p_max, r_max
        line["lps_per_s_new"] = line["lps"] / (res["new_ms"]["median"] * 1e-3)
        if not a.new_only and todo:
            got = {k: v.cpu().numpy() for k, v in out["new"].items()}
            same = 0
            for p, (leaves, _) in zip(todo, out["loop"]):
                mine = batch.region_diff_leaves(got, p)
                same += len(mine) == len(leaves) and all(k0 == k1 and np.array_equal(r0, r1)
                                                         for (k0, r0), (k1, r1) in zip(mine, leaves))
            line["same_leaves"], line["compared"] = int(same), len(todo)
            line["loop_lps"] = int(sum(s["lps"] for _, s in out["loop"]))
            scaled = res["loop_%d_ms" % len(todo)]["median"] * len([p for p in range(B) if sized["status"][p] == batch.RD_OK
                                                                    and pre["cell_off"][p + 1] > pre["cell_off"][p]]) / len(todo)
            line["loop_scaled_to_batch_ms"] = scaled
            line["speedup_median"] = scaled / res["new_ms"]["median"]
        print(json.dumps(line))
        sys.stdout.flush()


if __name__ == "__main__":
    main()
