#!/usr/bin/env python3
"""is_convex_batch / envelope_outer_batch (polytope_amd, csrc/plp_envelope.hip: the facet tests of envelope() for many
regions in one launch, one (region, member) entry per wavefront) against what there is without them.  All sides run
alternately in this process -- warm-up, then >= 20 repetitions each, every one ending in a device synchronise -- and each
shape prints as one JSON line with median, minimum and maximum in ms:

  (1) 10 000 regions of 4 members of (8, 3): half are a box cut into four by two planes (convex), half four random
      polytopes around nearby centres
  (2) 1 000 regions of 8 members of (10, 4): half are a box cut into eight slabs (convex), half eight random polytopes

  batch_ms          polytope_amd.is_convex_batch(regions) on 'hip' (caches of the regions and members cleared before
                    every repetition, outside the timing)
  loop_N_ms         (a) the loop of is_convex(region) over the first --loop-regions (100) regions; `loop_scaled_ms` scales
                    its median to the batch
  kernel_call_ms    the envelope stage alone: batch.envelope_outer_batch on device-resident tensors
  stacks_ms         (b) the honest alternative for that stage: every test stack [member j; -row ii of member i] built with
                    numpy and sent through ONE cheby_ball_batch (stack building included: it is part of that route);
                    `stacks_lp_only_ms` is the cheby_ball_batch call alone on the stacks built once

    python scripts/bench_envelope.py [--reps 20] [--warmup 3] [--rows 1,2] [--kernel-only]
Kernel times: `--kernel-only` under rocprofv3 --kernel-trace --stats."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402
import polytope_amd  # noqa: E402
import polytope_amd.polytope as pcm  # noqa: E402
from polytope_amd import batch, solvers  # noqa: E402


def stats(ts):
    return dict(median=float(np.median(ts)), min=float(np.min(ts)), max=float(np.max(ts)))


def alternate(fns, reps, warmup, before=None):
    """Every function of `fns` in turn, `reps` times, each call ending in a synchronise -> one stats dict per function.
    `before()` runs in front of every call, outside the timing."""
    ts = [[] for _ in fns]
    for r in range(warmup + reps):
        for fn, t in zip(fns, ts):
            if before is not None:
                before()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if r >= warmup:
                t.append((time.perf_counter() - t0) * 1e3)
    return [stats(t) for t in ts]


def unit(A, b):
    n = np.linalg.norm(A, axis=-1)
    return A / n[..., None], b / n


def make_regions(B, n_mem, m, d, seed):
    """B regions of n_mem members of m rows in R^d -> A[B, n_mem, m, d], b[B, n_mem, m]; even regions are a box cut into
    n_mem convex pieces (2d box rows + m - 2d cutting rows; for n_mem = 4 two planes, else slabs along axis 0 with the
    spare rows far outside), odd regions n_mem random polytopes (box + random cuts) around nearby centres."""
    rng = np.random.default_rng(seed)
    box = np.concatenate([np.eye(d), -np.eye(d)])
    spare = m - 2 * d
    A, b = np.zeros((B, n_mem, m, d)), np.zeros((B, n_mem, m))
    for k in range(B):
        c0 = rng.uniform(-1, 1, d)
        if k % 2 == 0 and n_mem == 4 and spare == 2:
            n1, n2 = rng.standard_normal((2, d))
            n1, n2 = n1 / np.linalg.norm(n1), n2 / np.linalg.norm(n2)
            for q, (s1, s2) in enumerate(((1, 1), (1, -1), (-1, 1), (-1, -1))):
                A[k, q] = np.concatenate([box, [s1 * n1, s2 * n2]])
                b[k, q] = np.concatenate([box @ c0 + 1.0, [s1 * (n1 @ c0), s2 * (n2 @ c0)]])
        elif k % 2 == 0:
            edges = np.linspace(-1.0, 1.0, n_mem + 1)
            far = rng.standard_normal((spare, d))
            far /= np.linalg.norm(far, axis=1, keepdims=True)
            for q in range(n_mem):
                bb = box @ c0 + 1.0
                bb[0], bb[d] = c0[0] + edges[q + 1], -(c0[0] + edges[q])
                A[k, q] = np.concatenate([box, far])
                b[k, q] = np.concatenate([bb, far @ c0 + 10.0])
        else:
            for q in range(n_mem):
                cuts = rng.standard_normal((spare, d))
                cuts /= np.linalg.norm(cuts, axis=1, keepdims=True)
                c = c0 + rng.uniform(-0.5, 0.5, d)
                A[k, q] = np.concatenate([box, cuts])
                b[k, q] = A[k, q] @ c + np.concatenate([np.ones(2 * d), rng.uniform(0.5, 0.9, spare)])
    return A, b


def build_stacks(A, b):
    """Every test stack of every region: [member j; -row ii of member i], i != j -> A3[T, m + 1, d], b3[T, m + 1]."""
    B, n, m, d = A.shape
    i, j = [v.ravel() for v in np.nonzero(~np.eye(n, dtype=bool))]          # the ordered pairs i != j
    top_A = np.broadcast_to(A[:, j][:, :, None], (B, len(j), m, m, d))       # [B, pair, ii, rows of j, d]
    top_b = np.broadcast_to(b[:, j][:, :, None], (B, len(j), m, m))
    neg_A, neg_b = -A[:, i][:, :, :, None, :], -b[:, i][:, :, :, None]       # [B, pair, ii, 1, d]
    A3 = np.concatenate([top_A, neg_A], axis=3).reshape(-1, m + 1, d)
    b3 = np.concatenate([top_b, neg_b], axis=3).reshape(-1, m + 1)
    return A3, b3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rows", default="1,2")
    ap.add_argument("--loop-regions", type=int, default=100)
    ap.add_argument("--kernel-only", action="store_true", help="the envelope kernel's call alone (profiling runs)")
    a = ap.parse_args()
    solvers.default_solver = "hip"
    dev = torch.device("cuda:0")
    shapes = {"1": ("10000 regions x 4 members of (8, 3)", (10000, 4, 8, 3, 81)),
              "2": ("1000 regions x 8 members of (10, 4)", (1000, 8, 10, 4, 82))}
    for row in a.rows.split(","):
        what, (B, n, m, d, seed) = shapes[row]
        A, b = unit(*make_regions(B, n, m, d, seed))
        regs = [pcm.Region([pcm.Polytope(A[k, q], b[k, q], normalize=False) for q in range(n)]) for k in range(B)]
        sub = regs[:a.loop_regions]
        flatA, flatb = A.reshape(B * n, m, d), b.reshape(B * n, m)
        reg_off = np.arange(0, B * n + 1, n, dtype=np.int32)
        targs = [torch.as_tensor(x, device=dev) for x in (flatA, flatb)] + [None, torch.as_tensor(reg_off, device=dev)]
        out = {}

        def reset():
            for r in regs:
                r.bbox = r.fulldim = r._chebXc = r._chebR = None
                for p in r.list_poly:
                    p.bbox = p.fulldim = p._chebXc = None
                    p._chebR = 0

        def kernel_call():
            out["kernel"] = batch.envelope_outer_batch(*targs)

        def stacks():
            A3, b3 = build_stacks(A, b)
            out["stacks"] = batch.cheby_ball_batch(A3, b3)

        def batch_call():
            out["batch"] = polytope_amd.is_convex_batch(regs)

        def loop():
            out["loop"] = [pcm.is_convex(r) for r in sub]

        if a.kernel_only:
            res = dict(zip(["kernel_call_ms"], alternate([kernel_call], a.reps, a.warmup)))
            print(json.dumps(dict(row=row, what=what, **res, lps=int(out["kernel"]["nlp"].sum().item()))))
            continue
        A3, b3 = build_stacks(A, b)
        t3 = [torch.as_tensor(x, device=dev) for x in (A3, b3)]

        def stacks_lp_only():
            out["stacks_lp"] = batch.cheby_ball_batch(*t3)

        fns = [batch_call, loop, kernel_call, stacks, stacks_lp_only]
        names = ["batch_ms", "loop_%d_ms" % len(sub), "kernel_call_ms", "stacks_ms", "stacks_lp_only_ms"]
        res = dict(zip(names, alternate(fns, a.reps, a.warmup, before=reset)))
        line = dict(row=row, what=what, **res)
        line["loop_scaled_ms"] = res["loop_%d_ms" % len(sub)]["median"] * B / len(sub)
        line["speedup_vs_loop"] = line["loop_scaled_ms"] / res["batch_ms"]["median"]
        line["kernel_vs_stacks"] = res["stacks_ms"]["median"] / res["kernel_call_ms"]["median"]
        line["kernel_vs_stacks_lp_only"] = res["stacks_lp_only_ms"]["median"] / res["kernel_call_ms"]["median"]
        k = {key: v.cpu().numpy() for key, v in out["kernel"].items()}
        line["lps_rule"], line["lps_brute"] = int(k["nlp"].sum()), int(A3.shape[0])
        line["status_counts"] = {int(s): int(v) for s, v in zip(*np.unique(k["status"], return_counts=True))}
        line["convex"] = int(sum(bool(v[0]) for v in out["batch"]))
        line["same_as_loop"] = int(sum(bool(x[0]) == bool(y[0]) for x, y in zip(out["batch"], out["loop"])))
        # the masks of route (b), read as the rule reads a radius
        R = np.where((out["stacks"]["status"] == 0) & (out["stacks"]["r"] >= 0), out["stacks"]["r"], 0.0)
        crossed = (R > 1e-7).reshape(B, n * (n - 1), m)
        i = np.nonzero(~np.eye(n, dtype=bool))[0]
        word = np.zeros((B, n), np.uint64)
        for q in range(n):
            outer_q = ~crossed[:, i == q].any(axis=1)
            word[:, q] = (outer_q * (np.uint64(1) << np.arange(m, dtype=np.uint64))[None, :]).sum(axis=1).astype(np.uint64)
        ok = k["status"].reshape(B, n) == batch.ENV_OK
        line["masks_equal_where_ok"] = bool(np.array_equal(word[ok], k["outer"].view(np.uint64).reshape(B, n)[ok]))
        print(json.dumps(line))
        sys.stdout.flush()


if __name__ == "__main__":
    main()
