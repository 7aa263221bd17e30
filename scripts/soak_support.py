#!/usr/bin/env python3
"""Soak of support_batch's per-LP function on the CPU, not part of the test suite: the HOST build of
polytope_amd/csrc/plp_support.hpp (tests/cabi/support_host.cpp -- the device's answers are its answers bit for bit,
tests/test_support_gpu.py) over the seven families of scripts/soak_lane.py: make, every LP against the oracle's simplex.

Per (family, seed): tests/support_host.py: soak_cases -- six shapes (d = 1..4, 16 / 32 / 64 row slots), 30 polytopes each,
centres from the oracle's ball LP (none: the polytope must come back as status 1), 7 random directions + -e_i shared and
the tie directions (row normals, sums of neighbouring ones, their negatives) per polytope.  Counted per family: LPs of
polytopes with a centre, handed back (status 1), WRONG: a status that is not the oracle's, a status 0 whose h is off by more
than 1e-9 max(1, |h|, |x_oracle|_max), whose x violates a row by more than that or whose c.x is not h to 1e-12.  Where h
differs from the oracle's, support_host.exact_support (rational arithmetic on the stored doubles) arbitrates: the answer is
wrong when it is beyond 1e-9 of the extent from the EXACT h, and counted as "oracle off" when it is within and the oracle is
not (the oracle, like HiGHS, reads entries <= 1e-9 as zero and accepts points 1e-9 outside a row).
The case builders and the host-build loader are the test suite's (tests/support_host.py), so the soak and the tests run
the same inputs.
Usage: python scripts/soak_support.py [seeds per family = 200] [first seed = 1000] [host library built elsewhere]"""
import multiprocessing as mp
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import support_host as sh  # noqa: E402

_L = None


def wrong_answers(case, layout, h, x, st):
    """[(polytope, direction, what, h, h_oracle)] of the LPs that are not handed back and not right."""
    C_, ost, oh, ox = case[layout]
    A, b, m = case["A"], case["b"], case["m"]
    B, K = st.shape
    Cb = np.broadcast_to(C_, (B,) + C_.shape) if C_.ndim == 2 else C_
    has = np.isfinite(case["xc"]).all(axis=1)
    out = []
    for p, j in np.argwhere(st != 1):
        what = None
        if not has[p] or st[p, j] != ost[p, j]:
            what = "status %d, oracle %d" % (st[p, j], ost[p, j])
            if has[p] and (st[p, j], ost[p, j]) in ((0, 3), (3, 0)):   # (the oracle calls an optimum beyond 1e9 x the data unbounded)
                he, xe = sh.exact_support(A[p, :m[p]], b[p, :m[p]], Cb[p, j], case["xc"][p])
                if st[p, j] == 3 and he is None:
                    what = "ORACLE OFF: unbounded in exact arithmetic, oracle h = %.17g" % oh[p, j]
                elif st[p, j] == 0 and he is not None:
                    xm = max(abs(float(v)) for v in xe)
                    ke = float(h[p, j] - he) / max(1.0, abs(h[p, j]), xm)
                    if abs(ke) <= 1e-9:
                        what = "ORACLE OFF: oracle 3, kernel %+.3g of the extent from the exact h, |x|_max %.3g" % (ke, xm)
        elif st[p, j] == 0:
            scale = max(1.0, abs(h[p, j]), ox[p, j])
            viol = np.max(A[p, :m[p]] @ x[p, j] - b[p, :m[p]], initial=-np.inf)
            if not abs(h[p, j] - oh[p, j]) <= 1e-9 * scale:
                # the oracle reads matrix entries <= 1e-9 as zero and accepts points 1e-9 outside a row (as HiGHS does): on rows
                # tilted by 1e-9 ITS h is off by a few 1e-9.  Exact rational arithmetic on the stored doubles arbitrates.
                he, xe = sh.exact_support(A[p, :m[p]], b[p, :m[p]], Cb[p, j], case["xc"][p])
                if he is None:
                    what = "status 0, unbounded in exact arithmetic"
                else:
                    se = max(1.0, abs(h[p, j]), max(abs(float(v)) for v in xe))
                    ke, oe = float(h[p, j] - he) / se, float(oh[p, j] - he) / se
                    what = "%s: kernel %+.3g, oracle %+.3g of the extent from the exact h" % (
                        "ORACLE OFF" if abs(ke) <= 1e-9 else "h off", ke, oe)
            elif not viol <= 1e-9 * scale:
                what = "row violated by %.3g" % viol
            elif not abs(Cb[p, j] @ x[p, j] - h[p, j]) <= 1e-12 * max(1.0, abs(h[p, j])):
                what = "c.x is not h"
        elif st[p, j] == 3 and h[p, j] != np.inf:
            what = "status 3 without h = inf"
        if what:
            out.append((int(p), int(j), what, float(h[p, j]), float(oh[p, j])))
    return out


def _task(args):
    global _L
    fam, seed, libpath = args
    from oracle import oracle as O
    if _L is None:
        _L = sh.load(libpath)
    n = back = 0
    wrong = []
    for case in sh.soak_cases(O, fam, seed):
        has = np.isfinite(case["xc"]).all(axis=1)
        for layout in ("shared", "own"):
            h, x, st = sh.run_case(_L, case, layout)
            n += int(has.sum()) * st.shape[1]
            back += int((st[has] == 1).sum())
            wrong += [(fam, seed, tuple(case["shape"]), layout) + w for w in wrong_answers(case, layout, h, x, st)]
    return fam, n, back, wrong


def main():
    seeds = int(sys.argv[1]) if len(sys.argv) > 1 else 200
    seed0 = int(sys.argv[2]) if len(sys.argv) > 2 else 1000
    from oracle import oracle as O
    O.build()
    tmp = tempfile.mkdtemp(prefix="soak_support_")
    libpath = sys.argv[3] if len(sys.argv) > 3 else sh.build(tmp, as_path=True)
    t0 = time.time()
    pool = mp.get_context("fork").Pool(max(1, min(16, (os.cpu_count() or 2) - 1)))
    tasks = [(fam, seed0 + s, libpath) for fam in sh.FAMILIES for s in range(seeds)]
    tot = {fam: [0, 0, []] for fam in sh.FAMILIES}
    for fam, n, back, wrong in pool.imap_unordered(_task, tasks, chunksize=4):
        tot[fam][0] += n
        tot[fam][1] += back
        tot[fam][2] += wrong
    pool.close()
    pool.join()
    nwrong = 0
    for fam in sh.FAMILIES:
        n, back, wrong = tot[fam]
        off = [w for w in wrong if w[6].startswith("ORACLE OFF")]   # the kernel is within 1e-9 of the exact h, the oracle is not
        wrong = [w for w in wrong if not w[6].startswith("ORACLE OFF")]
        nwrong += len(wrong)
        print("%-9s  %8d LPs   handed back %6d (%.2f %%)   wrong %d   (oracle off, kernel right by exact arithmetic: %d)" % (
            fam, n, back, 100.0 * back / max(n, 1), len(wrong), len(off)))
        for w in sorted(wrong)[:40] + sorted(off)[:int(os.environ.get("SOAK_SUPPORT_SHOW_OFF", "3"))]:
            print("      ", w)
    print("SUPPORT SOAK %s: seeds %d .. %d per family, %d wrong, %.0f s" % (
        "FAILED" if nwrong else "OK", seed0, seed0 + seeds - 1, nwrong, time.time() - t0), flush=True)
    return 1 if nwrong else 0


if __name__ == "__main__":
    sys.exit(main())
