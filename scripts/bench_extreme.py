#!/usr/bin/env python3
"""extreme_batch (polytope_amd.batch, csrc/plp_extreme.hip: the vertices of many small polytopes in one launch) against
the only way to get them without it: a loop over extreme(Polytope) with the 'hip' backend (per polytope a reduce, a
Chebyshev LP, a quickhull of the polar dual and a second reduce).  Both run alternately in this process -- warm-up, then
>= 20 repetitions each, every one ending in a device synchronise -- and each shape prints as one JSON line with median,
minimum and maximum in ms:

  (1) 10 000 x (16, 3)      (2) 10 000 x (12, 2)      (3) 1 000 x (16, 4)

`new`: extreme_batch(reduce=True) on device-resident torch tensors (reduce_batch, bbox_batch, the enumeration kernel and one
scalar read back for v_max); `new_raw`: extreme_batch(reduce=False, v_max given), the kernel alone behind its Python call.
`loop`: extreme() on the first --loop-polytopes (100) polytopes, each built afresh (extreme caches its result in the
object), scaled to the batch.  The vertex sets of the two paths are compared once per shape on those polytopes.

    python scripts/bench_extreme.py [--reps 20] [--warmup 3] [--rows 1,2,3] [--new-only]
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
from polytope_amd import solvers, synth  # noqa: E402


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


def same_vertices(V, R):
    """The batch's vertices of one polytope against extreme()'s rows (which repeat a degenerate vertex), as sets."""
    if R is None or not len(V):
        return R is None and not len(V)
    E = max(1.0, float(np.abs(R).max()))
    near = np.abs(V[:, None, :] - R[None, :, :]).max(axis=2) <= 1e-8 * E
    return bool(near.any(axis=1).all() and near.any(axis=0).all())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rows", default="1,2,3")
    ap.add_argument("--loop-polytopes", type=int, default=100)
    ap.add_argument("--new-only", action="store_true", help="extreme_batch alone (profiling runs)")
    a = ap.parse_args()
    solvers.default_solver = "hip"
    dev = torch.device("cuda:0")
    shapes = {"1": (10000, 16, 3), "2": (10000, 12, 2), "3": (1000, 16, 4)}
    for row in a.rows.split(","):
        B, m, d = shapes[row]
        A, b = synth.random_hpolytopes(B, m, d, seed=60 + int(row), bounded=True)
        At, bt = (torch.as_tensor(v, device=dev) for v in (A, b))
        n = min(a.loop_polytopes, B)
        out = {}

        def new():
            out["new"] = pa.extreme_batch(At, bt)

        v_raw = pa.batch._extreme_vmax(d, m)

        def new_raw():
            out["raw"] = pa.extreme_batch(At, bt, v_max=v_raw, reduce=False)

        def loop():
            out["loop"] = [pa.extreme(pa.Polytope(A[p].copy(), b[p].copy())) for p in range(n)]

        fns, names = [new, new_raw], ["new_ms", "new_raw_ms"]
        if not a.new_only:
            fns.append(loop)
            names.append("loop_%d_ms" % n)
        res = dict(zip(names, alternate(fns, a.reps, a.warmup)))
        line = dict(row=row, what="%d x (%d, %d)" % (B, m, d), **res)
        st = out["new"]["status"].cpu().numpy()
        cnt = out["new"]["count"].cpu().numpy()
        line["status_counts"] = {int(k): int(v) for k, v in zip(*np.unique(st, return_counts=True))}
        line["vertices_mean"] = float(cnt.mean())
        line["v_max"] = int(out["new"]["V"].shape[1])
        if not a.new_only:
            V = out["new"]["V"][:n].cpu().numpy()
            line["same_vertex_sets"] = int(sum(same_vertices(V[p, :cnt[p]], out["loop"][p]) for p in range(n)))
            line["compared"] = n
            scaled = res["loop_%d_ms" % n]["median"] * B / n
            line["loop_scaled_to_batch_ms"] = scaled
            line["speedup_median"] = scaled / res["new_ms"]["median"]
        print(json.dumps(line))
        sys.stdout.flush()


if __name__ == "__main__":
    main()
