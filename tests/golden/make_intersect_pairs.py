#!/usr/bin/env python3
"""Generate tests/golden/intersect_pairs.npz by IMPORTING the reference (tulip-control/polytope, scipy / HiGHS backend):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_intersect_pairs.py <path to a checkout of the reference>

Cell families and, for every listed pair (i, j), the reference's cells[i].intersect(cells[j]) (the default abs_tol):
  a          two 3 x 3 x 2 grids of unit boxes in d = 3, the second moved by half a cell: 18 + 18 cells, all 324 cross pairs
  b2 .. b9   four random bounded polytopes of 5..16 rows per d = 2, 3, 4, 5, 8, 9, each with three extra rows that are NOT
             normalised (norms 1e-3 .. 30); all 12 ordered pairs within a d
  c          pairs of unit boxes in d = 3 overlapping by 0, 1e-8, 1.9e-7, 2.1e-7 and 1e-6 (cells 2 k and 2 k + 1)
  d          five intervals in d = 1, all 20 ordered pairs
Per family `f`: f_A[n, m_max, d], f_b[n, m_max], f_m[n] (the cells as given to the constructor, zero padded), f_pairs[K, 2],
and the results packed the same way, f_rA[K, mo_max, d], f_rb[K, mo_max], f_rm[K] (0: the empty polytope), f_minrep[K].
The fixture is data only; the reference is needed at generation time, never by a test."""
import os
import sys

import numpy as np

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
B_DIMS = (2, 3, 4, 5, 8, 9)
C_OVERLAPS = (0.0, 1e-8, 1.9e-7, 2.1e-7, 1e-6)


def pack(members):
    m = np.array([a.shape[0] for a, _ in members], dtype=np.int32)
    d = members[0][0].shape[1]
    A, b = np.zeros((len(members), max(int(m.max()), 1), d)), np.zeros((len(members), max(int(m.max()), 1)))
    for k, (a, bb) in enumerate(members):
        A[k, :m[k]], b[k, :m[k]] = a, bb
    return A, b, m


def box(lo, hi):
    lo, hi = np.asarray(lo, float), np.asarray(hi, float)
    d = lo.size
    return np.vstack([np.eye(d), -np.eye(d)]), np.concatenate([hi, -lo])


def grid(shape, origin):
    idx = np.stack(np.meshgrid(*[np.arange(s) for s in shape], indexing="ij"), -1).reshape(-1, len(shape))
    return [box(i + origin, i + origin + 1.0) for i in idx.astype(float)]


def random_polytope(rng, d):
    """A bounded polytope around a centre near the origin: a simplex (d + 1 rows), random unit cuts up to 5..16 rows in all,
    the last three rows scaled by 1e-3 .. 30 (not normalised)."""
    total = int(rng.integers(max(5, d + 4), 17))
    c = rng.uniform(-0.25, 0.25, d)
    rows = [-np.eye(d), np.ones((1, d)) / np.sqrt(d)]
    extra = rng.standard_normal((total - d - 1, d))
    a = np.vstack(rows + [extra / np.linalg.norm(extra, axis=1, keepdims=True)])
    b = a @ c + rng.uniform(0.6, 1.4, total)
    scale = np.ones(total)
    scale[-3:] = 10.0 ** rng.uniform(-3, np.log10(30.0), 3)
    return a * scale[:, None], b * scale


def families():
    """{name: (members [(A, b)], pairs int32[K, 2])}"""
    rng = np.random.default_rng(20261020)
    out = {}
    ga, gb = grid((3, 3, 2), 0.0), grid((3, 3, 2), 0.5)
    out["a"] = (ga + gb, np.array([(i, 18 + j) for i in range(18) for j in range(18)], dtype=np.int32))
    for d in B_DIMS:
        out["b%d" % d] = ([random_polytope(rng, d) for _ in range(4)],
                          np.array([(i, j) for i in range(4) for j in range(4) if i != j], dtype=np.int32))
    mem = []
    for k, g in enumerate(C_OVERLAPS):
        mem += [box([0.0, 0.0, 5.0 * k], [1.0, 1.0, 5.0 * k + 1.0]), box([1.0 - g, 0.0, 5.0 * k], [2.0 - g, 1.0, 5.0 * k + 1.0])]
    out["c"] = (mem, np.array([(2 * k, 2 * k + 1) for k in range(len(C_OVERLAPS))], dtype=np.int32))
    iv = [box([lo], [hi]) for lo, hi in ((0.0, 1.0), (0.5, 2.0), (1.0, 3.0), (-1.0, 0.2), (5.0, 6.0))]
    out["d"] = (iv, np.array([(i, j) for i in range(5) for j in range(5) if i != j], dtype=np.int32))
    return out


def main(reference):
    sys.path.insert(0, reference)
    import polytope as ref  # noqa: E402  (the reference)
    assert os.path.abspath(ref.__file__).startswith(os.path.abspath(reference)), ref.__file__
    out = {}
    for name, (members, pairs) in families().items():
        cells = [ref.Polytope(a.copy(), b.copy()) for a, b in members]
        res, minrep = [], []
        for i, j in pairs:
            q = cells[i].intersect(cells[j])
            d = members[0][0].shape[1]
            res.append((np.asarray(q.A, float).reshape(-1, d), np.asarray(q.b, float).ravel()) if len(q.A) else
                       (np.zeros((0, d)), np.zeros(0)))
            minrep.append(bool(q.minrep))
        out[name + "_A"], out[name + "_b"], out[name + "_m"] = pack(members)
        out[name + "_pairs"] = pairs
        out[name + "_rA"], out[name + "_rb"], out[name + "_rm"] = pack(res)
        out[name + "_minrep"] = np.array(minrep, dtype=np.uint8)
        print("family %s: %d cells, %d pairs, %d non-empty, rows %s" % (name, len(members), len(pairs),
                                                                       int((out[name + "_rm"] > 0).sum()),
                                                                       sorted(set(out[name + "_rm"].tolist()))))
    assert out["c_rm"].tolist() == [0, 0, 0, 6, 6], out["c_rm"]
    np.savez_compressed(os.path.join(HERE, "intersect_pairs.npz"), **out)


if __name__ == "__main__":
    main(sys.argv[1])
