#!/usr/bin/env python3
"""distance_pairs (polytope_amd.batch, csrc/plp_pair_dist.hip: a GJK iteration per listed cell pair, two lanes per pair,
two support LPs per round) on device-resident torch tensors.  The routes of a row run alternately in this process --
warm-up, then >= 20 repetitions each, every one ending in a device synchronise -- and each row prints as one JSON line
with median, minimum and maximum in ms:

  (1) the 1000-cell d = 4 box grid (10 x 10 x 5 x 2): the candidate list of box_pairs plus as many random far pairs;
      beside it pair_verdicts on the same list (one Chebyshev LP per pair)
  (2) 10 000 random (16, 3) cells, each moved by a random offset, 100 000 random pairs; beside it the host build of the
      same source (tests/cabi/pair_dist_host.cpp) in a plain loop on one CPU core, timed on 100 pairs and scaled to the list
      (`cpu_scaled_ms`: an ESTIMATE)

Per row also the share of pairs the kernel hands back (`handback`, raw status 1) and the mean support rounds per pair, which
the kernel does not give out: the host build's count on the first 1000 pairs of the list (`rounds_mean_sample`).
Nothing here is a pass / fail threshold.

    python scripts/bench_distance_pairs.py [--reps 20] [--warmup 3] [--rows 1,2]"""
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
from polytope_amd import batch, synth  # noqa: E402
from bench_support import alternate  # noqa: E402


def host_side(L, ph, A, b, xc, P):
    """The host build: (ms for the whole list scaled from 100 pairs, mean rounds of the settled among the first 1000)."""
    t0 = time.perf_counter()
    ph.run(L, A, b, xc, P[:100])
    ms = (time.perf_counter() - t0) * 1e3 * len(P) / min(100, len(P))
    s = ph.run(L, A, b, xc, P[:1000])
    ok = s["status"] == 0
    return ms, float(s["rounds"][ok].mean()) if ok.any() else float("nan")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rows", default="1,2")
    a = ap.parse_args()
    rows = {int(r) for r in a.rows.split(",")}
    dev = torch.device("cuda:0")
    import pair_dist_host as ph
    L = ph.build(tempfile.mkdtemp(prefix="pair_dist_host_"))
    rng = np.random.default_rng(0)
    if 1 in rows:
        edges = [np.linspace(0.0, 1.0, n + 1) for n in (10, 10, 5, 2)]   # 10 x 10 x 5 x 2 = 1000 cells
        lo = np.array([[edges[k][i[k]] for k in range(4)] for i in np.ndindex(10, 10, 5, 2)])
        hi = np.array([[edges[k][i[k] + 1] for k in range(4)] for i in np.ndindex(10, 10, 5, 2)])
        A, b, xc = ph.boxes_as_cells(lo, hi)
        n = A.shape[0]
        cand = batch.box_pairs(lo, hi)["pairs"]
        far = np.stack([rng.integers(0, n, len(cand)), rng.integers(0, n, len(cand))], axis=1)
        far = far[far[:, 0] != far[:, 1]]
        P = np.ascontiguousarray(np.vstack([cand, far]), dtype=np.int32)
        At, bt, xt, Pt = (torch.as_tensor(v).to(dev) for v in (A, b, xc, P))
        raw = batch.distance_pairs(At, bt, Pt, xc=xt, resolve=False)
        new, ver = alternate([lambda: batch.distance_pairs(At, bt, Pt, xc=xt, resolve=False),
                              lambda: batch.pair_verdicts(At, bt, Pt)], a.reps, a.warmup)
        cpu_ms, rounds = host_side(L, ph, A, b, xc, P)
        print(json.dumps(dict(row=1, cells=n, d=4, m=8, K=len(P), candidates=len(cand), distance_pairs_ms=new, pair_verdicts_ms=ver,
                              handback=float((raw["status"] == 1).double().mean()), rounds_mean_sample=rounds,
                              cpu_scaled_ms=cpu_ms)), flush=True)
    if 2 in rows:
        n, m, d, K = 10000, 16, 3, 100000
        A, b = synth.random_hpolytopes(n, m, d, seed=2)
        b = ph.translated(A, b, rng, reach=8.0)
        i = rng.integers(0, n, K)
        P = np.ascontiguousarray(np.stack([i, (i + rng.integers(1, n, K)) % n], axis=1), dtype=np.int32)
        At, bt, Pt = (torch.as_tensor(v).to(dev) for v in (A, b, P))
        xt = pa.cheby_ball_batch(At, bt)["xc"]
        raw = batch.distance_pairs(At, bt, Pt, xc=xt, resolve=False)
        (new,) = alternate([lambda: batch.distance_pairs(At, bt, Pt, xc=xt, resolve=False)], a.reps, a.warmup)
        cpu_ms, rounds = host_side(L, ph, A, b, xt.cpu().numpy(), P)
        print(json.dumps(dict(row=2, cells=n, d=d, m=m, K=K, distance_pairs_ms=new, handback=float((raw["status"] == 1).double().mean()),
                              rounds_mean_sample=rounds, cpu_scaled_ms=cpu_ms, cpu_scaled_is="an estimate: 100 pairs on one core, scaled")),
              flush=True)


if __name__ == "__main__":
    main()
