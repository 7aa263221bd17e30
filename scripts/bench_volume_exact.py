#!/usr/bin/env python3
"""volume_exact_batch (polytope_amd.batch, csrc/plp_volume_exact.hip: exact volumes and facet areas of many small polytopes
in one launch) against volume_batch, the Monte-Carlo estimate it stands beside, at the reference's default sample count
(500 / 3000 / 10000 for d = 2 / 3 / 4).  All run alternately in this process -- warm-up, then >= 20 repetitions each, every
one ending in a device synchronise -- and each shape prints as one JSON line with median, minimum and maximum in ms:

  (1) 10 000 x (16, 3)      (2) 10 000 x (12, 2)      (3) 1 000 x (16, 4)

`exact`: volume_exact_batch(reduce=True) on device-resident torch tensors (reduce_batch, bbox_batch, the kernel);
`exact_raw`: volume_exact_batch(reduce=False), the kernel alone behind its Python call; `sampled`: volume_batch with one
seed for the call, the stream every polytope then draws (bbox_batch, the sampling kernel, the counts read back).
`worst_sigmas`: the largest |exact - sampled| over the batch in units of the sampling deviation box sqrt(p (1 - p) / N),
p = exact / box -- a check that the two measure the same thing; `rel_sigma_median`: that deviation over the volume.

    python scripts/bench_volume_exact.py [--reps 20] [--warmup 3] [--rows 1,2,3] [--new-only]
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
from polytope_amd import synth  # noqa: E402


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rows", default="1,2,3")
    ap.add_argument("--new-only", action="store_true", help="volume_exact_batch alone (profiling runs)")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    shapes = {"1": (10000, 16, 3), "2": (10000, 12, 2), "3": (1000, 16, 4)}
    for row in a.rows.split(","):
        B, m, d = shapes[row]
        A, b = synth.random_hpolytopes(B, m, d, seed=70 + int(row), bounded=True)
        At, bt = (torch.as_tensor(v, device=dev) for v in (A, b))
        out = {}

        def exact():
            out["exact"] = pa.volume_exact_batch(At, bt)

        def exact_raw():
            out["raw"] = pa.volume_exact_batch(At, bt, reduce=False)

        def sampled():
            out["mc"] = pa.volume_batch(At, bt, seed=1000 * int(row))

        fns, names = [exact, exact_raw], ["exact_ms", "exact_raw_ms"]
        if not a.new_only:
            fns.append(sampled)
            names.append("sampled_ms")
        res = dict(zip(names, alternate(fns, a.reps, a.warmup)))
        line = dict(row=row, what="%d x (%d, %d)" % (B, m, d), **res)
        st = out["exact"]["status"].cpu().numpy()
        vol = out["exact"]["volume"].cpu().numpy()
        line["status_counts"] = {int(k): int(v) for k, v in zip(*np.unique(st, return_counts=True))}
        ok = st == 0
        raw = out["raw"]["volume"].cpu().numpy()
        line["reduce_vs_raw_rel_max"] = float(np.max(np.abs(raw[ok] - vol[ok]) / vol[ok]))
        if not a.new_only:
            mc = out["mc"]
            N = int(mc["nsamples"])
            box = np.prod(mc["ub"].cpu().numpy() - mc["lb"].cpu().numpy(), axis=1)
            vmc = mc["volume"].numpy()
            use = ok & np.isfinite(vmc)
            p = np.clip(vol[use] / box[use], 0.0, 1.0)
            sg = box[use] * np.sqrt(np.maximum(p * (1 - p), 1.0 / N) / N)
            line["nsamples"] = N
            line["compared"] = int(use.sum())
            line["worst_sigmas"] = float(np.max(np.abs(vol[use] - vmc[use]) / sg))
            line["rel_sigma_median"] = float(np.median(sg / vol[use]))
            line["sampled_over_exact_median"] = res["sampled_ms"]["median"] / res["exact_ms"]["median"]
        print(json.dumps(line))
        sys.stdout.flush()


if __name__ == "__main__":
    main()
