#!/usr/bin/env python3
"""support_batch (polytope_amd.batch, csrc/plp_support.hip: K directions per polytope, the rows staged once) against the
only way to do the same work without it: lpsolve_batch on the replicated form, one copy of the rows per direction.  Both
run alternately in this process on device-resident torch tensors -- warm-up, then >= 20 repetitions each, every one
ending in a device synchronise -- and each shape prints as one JSON line with median, minimum and maximum in ms:

  (1) 10 000 x (16, 3) x K = 64 directions shared by all polytopes
  (2)  1 000 x (32, 4) x K = 256 directions per polytope
  (3) 100 000 x (16, 3) x K = 6, C = +-I, with bbox_batch (the one multi-objective shape with a kernel of its own) beside it

`new`: support_batch with the centres given; `new_with_centres`: xc=None, cheby_ball_batch inside the call.  The replicated
tensors G[B K, m, d], h[B K, m], c[B K, d] are built before the clock starts (the expansion itself is not charged to the
old path).  The two paths' optima are compared once per shape (max_rel_diff).

    python scripts/bench_support.py [--reps 20] [--warmup 3] [--rows 1,2,3] [--new-only]
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
    ap.add_argument("--new-only", action="store_true", help="support_batch alone (profiling runs)")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    shapes = {"1": (10000, 16, 3, 64, "shared"), "2": (1000, 32, 4, 256, "per-polytope"), "3": (100000, 16, 3, 6, "axes")}
    for row in a.rows.split(","):
        B, m, d, K, kind = shapes[row]
        A, b = synth.random_hpolytopes(B, m, d, seed=40 + int(row), bounded=True)
        rng = np.random.default_rng(int(row))
        if kind == "shared":
            C = rng.standard_normal((K, d))
        elif kind == "per-polytope":
            C = rng.standard_normal((B, K, d))
        else:
            C = np.vstack([np.eye(d), -np.eye(d)])
        At, bt, Ct = (torch.as_tensor(v, device=dev) for v in (A, b, C))
        xc = pa.cheby_ball_batch(At, bt)["xc"]
        out = {}

        def new():
            out["new"] = pa.support_batch(At, bt, Ct, xc=xc, points=True)

        def new_with_centres():
            out["newc"] = pa.support_batch(At, bt, Ct, points=True)

        fns, names = [new, new_with_centres], ["new_ms", "new_with_centres_ms"]
        if not a.new_only:
            # the replicated form: LP (p, j) = row p K + j
            G = At[:, None].expand(B, K, m, d).reshape(B * K, m, d).contiguous()
            hh = bt[:, None].expand(B, K, m).reshape(B * K, m).contiguous()
            cc = (-(Ct[None].expand(B, K, d) if Ct.dim() == 2 else Ct)).reshape(B * K, d).contiguous()

            def old():
                out["old"] = pa.lpsolve_batch(cc, G, hh)
            fns.append(old)
            names.append("old_ms")
            if kind == "axes":
                def box():
                    out["box"] = pa.bbox_batch(At, bt)
                fns.append(box)
                names.append("bbox_batch_ms")
        res = dict(zip(names, alternate(fns, a.reps, a.warmup)))
        line = dict(row=row, what="%d x (%d, %d) x K = %d %s directions" % (B, m, d, K, kind), lps=B * K, **res)
        st = out["new"]["status"]
        line["status_nonzero"] = int((st != 0).sum())
        if not a.new_only:
            hn, ho = out["new"]["h"].reshape(-1), -out["old"]["fun"]
            ok = (st.reshape(-1) == 0) & (out["old"]["status"] == 0)
            line["max_rel_diff"] = float(((hn - ho).abs() / hn.abs().clamp(min=1.0))[ok].max())
            line["speedup_median"] = res["old_ms"]["median"] / res["new_ms"]["median"]
            line["replicated_rows_mb"] = G.numel() * 8 / 1e6
        print(json.dumps(line))
        sys.stdout.flush()


if __name__ == "__main__":
    main()
