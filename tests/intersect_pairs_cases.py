"""What tests/test_intersect_pairs_api.py (CPU, scipy backend) and tests/test_intersect_pairs_gpu.py share: the fixture
tests/golden/intersect_pairs.npz (generated from the reference by tests/golden/make_intersect_pairs.py) and the comparison
of a result with the reference's."""
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAMILIES = ("a", "b2", "b3", "b4", "b5", "b8", "b9", "c", "d")
PARITY = 1e-9   # the project's parity bound against the reference's arrays


def load_fixture():
    """{family: dict(A, b, m, pairs, rA, rb, rm, minrep)}"""
    z = np.load(os.path.join(ROOT, "tests", "golden", "intersect_pairs.npz"))
    return {f: {k: z["%s_%s" % (f, k)] for k in ("A", "b", "m", "pairs", "rA", "rb", "rm", "minrep")} for f in FAMILIES}


def cells_of(pa, fam):
    """The family's cells as Polytopes of the package `pa` (the constructor normalises, as the reference's did)."""
    return [pa.Polytope(fam["A"][p, :fam["m"][p]].copy(), fam["b"][p, :fam["m"][p]].copy()) for p in range(len(fam["m"]))]


def differs_from_fixture(fam, t, q):
    """None, or in a few words how the Polytope q differs from the reference's result for pair t: the same number of rows
    in the same order, entries within PARITY, the same minrep."""
    mo = int(fam["rm"][t])
    rows = 0 if q.A.size == 0 else q.A.shape[0]
    if rows != mo:
        return "%d rows, the reference has %d" % (rows, mo)
    if mo == 0:
        return None
    err = max(float(np.abs(q.A - fam["rA"][t, :mo]).max()), float(np.abs(q.b - fam["rb"][t, :mo]).max()))
    if not err <= PARITY:
        return "rows differ by %.3g" % err
    if bool(q.minrep) != bool(fam["minrep"][t]):
        return "minrep %s, the reference has %s" % (q.minrep, bool(fam["minrep"][t]))
    return None
