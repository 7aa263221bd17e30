"""tests/golden/found/support/dup.npz: the three polytopes of the soak family `dup` (rows a hair apart) on which support_batch's
walk ended on a feasible vertex that is not the optimum and reported status 0 (four LPs; tests/support_host.py: FOUND), with
their directions, the oracle's Chebyshev centre and, per direction, the oracle's status and h (scipy / HiGHS agrees with it
on the four to every printed digit).
    python tests/golden/make_support_found.py      (regenerates the inputs from the generator stream of FOUND_SHAPES)"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import support_host as sh  # noqa: E402
from oracle import oracle as O  # noqa: E402

O.build()
out = {}
for seed, shape, p, j in sh.FOUND:
    key = "s%d_m%d_p%d" % (seed, shape[0], p)
    if "A_" + key in out:
        continue
    case = sh.soak_cases(O, "dup", seed, sh.FOUND_SHAPES)[sh.FOUND_SHAPES.index(shape)]
    C_, ost, oh, _ = case["shared"]
    out["A_" + key], out["b_" + key], out["xc_" + key] = case["A"][p], case["b"][p], case["xc"][p]
    out["C_" + key], out["status_" + key], out["h_" + key] = C_, ost[p], oh[p]
    try:
        from scipy.optimize import linprog
        for jj in range(C_.shape[0]):
            rs = linprog(-C_[jj], case["A"][p], case["b"][p], bounds=(None, None))
            assert rs.status == 0 and abs(-rs.fun - oh[p, jj]) <= 1e-7 * max(1.0, abs(oh[p, jj])), (key, jj, -rs.fun, oh[p, jj])
    except ImportError:
        pass
os.makedirs(os.path.join(ROOT, "tests", "golden", "found", "support"), exist_ok=True)
np.savez_compressed(os.path.join(ROOT, "tests", "golden", "found", "support", "dup.npz"), **out)
print({k: v.shape for k, v in out.items()})

# tests/golden/found/support/oracle_off.npz: the LPs of scripts/soak_support.py's `dup` seeds 1000 .. 1199 (and of seed 14) on
# which the ORACLE is more than 1e-9 of the extent from the exact optimum (support_host.exact_support: rational arithmetic on
# the stored doubles) -- it reads matrix entries <= 1e-9 as zero and accepts points 1e-9 outside a row, or calls an optimum
# at a vertex 1e9 away unbounded -- with that exact optimum, rounded to double, and the extent max(1, |h|, |x_exact|_max).
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import tempfile  # noqa: E402
import soak_support as SS  # noqa: E402

L = sh.build(tempfile.mkdtemp())
finds = []
for seed in [14] + list(range(1000, 1200)):
    for case in sh.soak_cases(O, "dup", seed):
        for layout in ("shared", "own"):
            h, x, st = sh.run_case(L, case, layout)
            C_ = case[layout][0]
            for p, j, what, _, _ in SS.wrong_answers(case, layout, h, x, st):
                assert what.startswith("ORACLE OFF"), (seed, case["shape"], layout, p, j, what)
                c = C_[j] if C_.ndim == 2 else C_[p, j]
                A, b = case["A"][p], case["b"][p]
                he, xe = sh.exact_support(A, b, c, case["xc"][p])
                ext = max(1.0, abs(float(he)), max(abs(float(v)) for v in xe))
                finds.append(("s%d_m%d_d%d_%s_p%d_j%d" % (seed, A.shape[0], A.shape[1], layout, p, j), A, b, c, case["xc"][p], float(he), ext))
off = {"names": np.array([f[0] for f in finds])}
for d in sorted({f[1].shape for f in finds}):
    sel = [f for f in finds if f[1].shape == d]
    tag = "m%d_d%d" % d
    off["idx_" + tag] = np.array([[f[0] for f in finds].index(g[0]) for g in sel])
    for k, name in ((1, "A"), (2, "b"), (3, "c"), (4, "xc")):
        off[name + "_" + tag] = np.stack([g[k] for g in sel])
off["h_exact"] = np.array([f[5] for f in finds])
off["extent"] = np.array([f[6] for f in finds])
np.savez_compressed(os.path.join(ROOT, "tests", "golden", "found", "support", "oracle_off.npz"), **off)
print(len(finds), "LPs where the oracle is off;", {k: v.shape for k, v in off.items()})
