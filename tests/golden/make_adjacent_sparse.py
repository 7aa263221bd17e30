#!/usr/bin/env python3
"""Generate tests/golden/adjacent_sparse.npz by IMPORTING the reference (tulip-control/polytope, scipy / HiGHS backend):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_adjacent_sparse.py <path to a checkout of the reference>

For each cell family of tests/box_pairs_host.py: fixture_families() -- (a) the 4 x 4 x 4 grid of unit boxes, (b) a
3 x 3 x 2 x 2 grid in d = 4, (c) 40 random bounded polytopes of 6..16 rows scattered in d = 3, (d) pairs of boxes 0, 1e-8,
1.7e-7, 1.9e-7, 2.1e-7 and 1e-6 apart -- the cells and the reference's is_adjacent(p, q) (overlap=True, the default
abs_tol; what find_adjacent_regions asks, prop2partition.py:57-61) on EVERY pair, as a symmetric uint8 matrix with ones on
the diagonal.  The fixture is data only; the reference is needed at generation time, never by a test."""
import os
import sys

import numpy as np

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))           # tests/
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))


def main(reference):
    from box_pairs_host import fixture_families, grid_cells, grid_touching
    fam = fixture_families()
    sys.path.insert(0, reference)
    import polytope as ref  # noqa: E402  (the reference)
    assert os.path.abspath(ref.__file__).startswith(os.path.abspath(reference)), ref.__file__
    out = {}
    for name, (A, b, m) in fam.items():
        n = A.shape[0]
        cells = [ref.Polytope(A[p, :(A.shape[1] if m is None else m[p])].copy(), b[p, :(A.shape[1] if m is None else m[p])].copy())
                 for p in range(n)]
        adj = np.eye(n, dtype=np.uint8)
        for i in range(n):
            for j in range(i):
                adj[i, j] = adj[j, i] = 1 if ref.is_adjacent(cells[i], cells[j]) else 0
        out[name + "_A"], out[name + "_b"] = A, b
        out[name + "_m"] = np.zeros(0, np.int32) if m is None else m
        out[name + "_adj"] = adj
        print("family %s: %d cells, %d pairs, %d adjacent" % (name, n, n * (n - 1) // 2, int(np.tril(adj, -1).sum())))
    # the 4 x 4 x 4 grid: exactly the touching pairs (faces, edges and corners) are adjacent
    _, _, idx = grid_cells((4, 4, 4))
    ii, jj = np.nonzero(np.tril(out["a_adj"], -1))
    assert np.array_equal(np.stack([ii, jj], 1), grid_touching(idx)), "family a: not the touching pairs"
    np.savez_compressed(os.path.join(HERE, "adjacent_sparse.npz"), **out)


if __name__ == "__main__":
    main(sys.argv[1])
