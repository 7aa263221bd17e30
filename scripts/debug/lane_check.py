"""GPU: reduce_lane_kernel (one LP per lane, plp_reduce_lane.hpp) against the lane-group kernels and the oracle, and its
timing next to theirs.   gpurun -- 'python scripts/debug/lane_check.py [lib.so ...]'"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def main():
    import torch
    import polytope_amd as pa
    from polytope_amd.synth import random_hpolytopes
    from oracle import oracle as O
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    dev = torch.device("cuda:0")

    def run(A, b, lane, m=None):
        os.environ["PLP_REDUCE_LANE"] = "1" if lane else "0"
        res = pa.reduce_batch(torch.as_tensor(A).to(dev), torch.as_tensor(b).to(dev),
                              None if m is None else torch.as_tensor(m).to(dev))
        torch.cuda.synchronize()
        return {k: v.cpu().numpy() for k, v in res.items()}

    ok = True
    timing_only = os.environ.get("PLP_LANE_CHECK_TIMING") == "1"
    # ---- parity: lane vs lane-group kernels (bitwise on every output), and vs the oracle
    for (B, m, d, seed) in [] if timing_only else [(20000, 16, 3, 0), (5000, 16, 3, 7), (3000, 12, 3, 3), (3000, 16, 2, 1), (3000, 9, 2, 2),
                            (2000, 6, 1, 4), (4099, 16, 3, 11)]:
        A, b = random_hpolytopes(B, m, d, seed=seed)
        r1, r0 = run(A, b, True), run(A, b, False)
        same = all(np.array_equal(r1[k], r0[k]) for k in ("keep", "flags", "nlp")) and \
            np.array_equal(r1["r"].view(np.int64), r0["r"].view(np.int64)) and \
            np.array_equal(r1["xc"].view(np.int64), r0["xc"].view(np.int64))
        Rr = O.reduce_batch(A, b)
        vs_or = np.array_equal(r1["keep"].view(np.uint64), Rr["keep"]) and np.array_equal(r1["flags"], Rr["flags"]) and \
            np.array_equal(r1["nlp"], Rr["nlp"]) and float(np.abs(r1["r"] - Rr["r"]).max()) <= 1e-9
        print("parity", (B, m, d), "lane == lane-group:", same, " lane == oracle:", vs_or, flush=True)
        ok = ok and same and vs_or
    if timing_only:
        return timing(torch, pa, random_hpolytopes, dev)
    # the latency shapes (8 / 4 polytopes per wavefront) and the mixed launch against the 16-per-wavefront form
    for (B, m, d, seed) in [(9000, 16, 3, 2), (5000, 13, 3, 5), (4000, 16, 2, 1), (3000, 5, 1, 9), (70001, 16, 3, 4)]:
        A, b = random_hpolytopes(B, m, d, seed=seed)
        os.environ["PLP_REDUCE_LANE_GS"] = "4"
        ref = run(A, b, True)
        outs = {}
        for gs in ("8", "16"):
            os.environ["PLP_REDUCE_LANE_GS"] = gs
            outs[gs] = run(A, b, True)
        del os.environ["PLP_REDUCE_LANE_GS"]
        outs["default"] = run(A, b, True)
        for k_, o in outs.items():
            same = all(np.array_equal(o[k], ref[k]) for k in ("keep", "flags", "nlp")) and \
                np.array_equal(o["r"].view(np.int64), ref["r"].view(np.int64)) and np.array_equal(o["xc"].view(np.int64), ref["xc"].view(np.int64))
            print("shape", (B, m, d), "GS", k_, "== GS 4:", same, flush=True)
            ok = ok and same
    # unbounded-allowed variant, ragged row counts
    A, b = random_hpolytopes(6000, 16, 3, seed=5, bounded=False)
    rng = np.random.default_rng(0)
    mm = rng.integers(1, 17, size=6000).astype(np.int32)
    r1, r0 = run(A, b, True, mm), run(A, b, False, mm)
    same = all(np.array_equal(r1[k], r0[k]) for k in ("keep", "flags", "nlp"))
    bad = 0
    for k in range(0, 6000, 3):
        o = O.reduce(A[k, :mm[k]], b[k, :mm[k]])
        bad += int(o["mask"] != int(r1["keep"][k]) or o["flags"] != int(r1["flags"][k]) or o["nlp"] != int(r1["nlp"][k]))
    print("parity ragged/unbounded: lane == lane-group:", same, " oracle mismatches:", bad, flush=True)
    ok = ok and same and bad == 0
    try:
        from structured_cases import structured_polytopes
        As, bs, fam = structured_polytopes(8192)
        r1, r0 = run(As, bs, True), run(As, bs, False)
        Rr = O.reduce_batch(As, bs)
        print("structured", As.shape[0], "lane == lane-group:", all(np.array_equal(r1[k], r0[k]) for k in ("keep", "flags", "nlp")),
              " lane == oracle:", np.array_equal(r1["keep"].view(np.uint64), Rr["keep"]) and np.array_equal(r1["nlp"], Rr["nlp"])
              and np.array_equal(r1["flags"], Rr["flags"]), flush=True)
    except Exception as e:  # the fixture module has another interface: say so, the random cases above still count
        print("structured cases skipped:", repr(e))
    timing(torch, pa, random_hpolytopes, dev)
    print("ALL OK" if ok else "MISMATCH")


def timing(torch, pa, random_hpolytopes, dev):
    NB = 6
    full = [random_hpolytopes(100000, 16, 3, seed=i) for i in range(NB)]
    for B in (100000, 50000, 25000, 12500, 6000, 3000):
        devb = [(torch.as_tensor(A_[:B]).to(dev), torch.as_tensor(b_[:B]).to(dev)) for A_, b_ in full]
        line = "B=%6d " % B
        for lane in (0, 1, 4, 8, 16):
            os.environ["PLP_REDUCE_LANE"] = "1" if lane else "0"
            os.environ.pop("PLP_REDUCE_LANE_GS", None)
            if lane > 1:
                os.environ["PLP_REDUCE_LANE_GS"] = str(lane)
            for k in range(5):
                pa.reduce_batch(*devb[k % NB])
            best = 1e9
            for rep in range(3):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for k in range(60):
                    pa.reduce_batch(*devb[k % NB])
                e1.record()
                torch.cuda.synchronize()
                best = min(best, e0.elapsed_time(e1) / 60)
            line += " %s %.4f" % ({0: "groups", 1: "lane"}.get(lane, "GS%d" % lane), best)
        os.environ.pop("PLP_REDUCE_LANE_GS", None)
        print(line, flush=True)


if __name__ == "__main__":
    libs = sys.argv[1:] or [None]
    if len(libs) == 1 and libs[0] is None:
        main()
    else:
        import subprocess
        for lib in libs:
            print("=====", lib, flush=True)
            env = dict(os.environ)
            if lib != "in-tree":
                env["PLP_LIB"] = os.path.abspath(lib)
            subprocess.run([sys.executable, os.path.abspath(__file__)], env=env)
