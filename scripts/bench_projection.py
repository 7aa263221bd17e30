#!/usr/bin/env python3
"""projection_batch (Fourier-Motzkin on the device, polytope_amd/batch.py) on batches of TuLiP-shaped polytopes -- a
state box, an input box and mt target rows through x+ = Ax + Bu, projected onto the states -- at (n, k, mt) = (3, 1, 8)
and (4, 2, 10).  Prints one JSON line per shape: ms per batch (warm-up, then >= 20 timed repetitions, each ending in a
device synchronise), launches and device-to-host bytes per step, the parity count against per-polytope projection() on
'hip', and the per-call projection() loop on 'hip' and on 'scipy' (a sample, extrapolated to the batch).

    python scripts/bench_projection.py [--B 10000] [--reps 20] [--warmup 3] [--sample 50]
Kernel times: run the same under rocprofv3 --kernel-trace --stats."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402
import polytope_amd as pa  # noqa: E402
from polytope_amd import solvers, batch  # noqa: E402
from polytope_amd import polytope as alg  # noqa: E402
from test_projection_gpu import tulip_batch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=10000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--sample", type=int, default=50)
    ap.add_argument("--shapes", default="3,1,8;4,2,10")
    a = ap.parse_args()
    solvers.default_solver = "hip"
    dev = torch.device("cuda:0")
    for shp in a.shapes.split(";"):
        n, k, mt = (int(v) for v in shp.split(","))
        rng = np.random.default_rng(100 + n * 10 + k)
        A, b = tulip_batch(rng, a.B, n, k, mt)
        At, bt = torch.as_tensor(A, device=dev), torch.as_tensor(b, device=dev)
        dim = list(range(1, n + 1))
        for _ in range(a.warmup):
            pa.projection_batch(At, bt, dim)
        torch.cuda.synchronize()
        times = []
        phases = {}   # phase -> host wall ms of each repetition (each phase ends in a synchronising copy)
        for _ in range(a.reps):
            t0 = time.perf_counter()
            res = pa.projection_batch(At, bt, dim)
            torch.cuda.synchronize()
            times.append((time.perf_counter() - t0) * 1e3)
            for s_ in batch.fm_stats.get("steps", []):
                phases.setdefault(s_["step"], []).append(s_["ms"])
        steps = [dict(s) for s in batch.fm_stats.get("steps", [])]
        for s_ in steps:
            ms = phases.get(s_["step"], [])
            s_.pop("ms", None)
            s_["ms_median"], s_["ms_min"], s_["ms_max"] = (float(np.median(ms)), float(np.min(ms)), float(np.max(ms))) \
                if ms else (0.0, 0.0, 0.0)
        st = res["status"].cpu().numpy()
        Ah, bh, mh = res["A"].cpu().numpy(), res["b"].cpu().numpy(), res["m"].cpu().numpy()
        idx = rng.choice(a.B, min(a.sample, a.B), replace=False)
        same = 0
        t0 = time.perf_counter()
        for t in idx:
            Q = alg.projection(pa.Polytope(A[t].copy(), b[t].copy(), normalize=False), dim, solver="fm")
            if Q.A.size == 0:
                same += int(st[t] == 1)
            else:
                same += int(st[t] == 0 and np.array_equal(Ah[t, :mh[t]], Q.A) and np.array_equal(bh[t, :mh[t]], Q.b))
        hip_ms = (time.perf_counter() - t0) * 1e3 / len(idx)
        solvers.default_solver = "scipy"
        ns = max(1, min(10, len(idx)))
        t0 = time.perf_counter()
        for t in idx[:ns]:
            alg.projection(pa.Polytope(A[t].copy(), b[t].copy(), normalize=False), dim, solver="fm")
        scipy_ms = (time.perf_counter() - t0) * 1e3 / ns
        solvers.default_solver = "hip"
        print(json.dumps(dict(
            shape=[n, k, mt], B=a.B, ms_per_batch_median=float(np.median(times)), ms_per_batch_min=float(np.min(times)),
            reps=a.reps, per_polytope_us=float(np.median(times)) * 1e3 / a.B, steps=steps, routed=int(res["routed"]),
            reexamined=int(res["reexamined"]), status_counts=np.bincount(st, minlength=4).tolist(),
            parity=[same, len(idx)], per_call_hip_ms=hip_ms, per_call_scipy_ms=scipy_ms,
            per_call_hip_batch_ms_extrapolated=hip_ms * a.B, per_call_scipy_batch_ms_extrapolated=scipy_ms * a.B)))
        sys.stdout.flush()


if __name__ == "__main__":
    main()
