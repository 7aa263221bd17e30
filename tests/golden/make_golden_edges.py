#!/usr/bin/env python3
"""g32_edges_d{1,2,3,4}.json.gz and g33_objects.json.gz -- what the reference itself returns (or the class of what it
raises) on the cases of tests/edge_cases.py, for tests/test_edge_objects.py (CPU, 'scipy' backend) and
tests/test_edge_objects_gpu.py ('hip' backend):

  g32_edges_d<d>   the 17 sets of menu_extended(d) -- empty, boxes (shifted, touching, apart, tiny, under 32 redundant rows,
                   with rows scaled by 1e-3 .. 1e3, translated by 100), half-space, slab, flat, infeasible, open cone,
                   duplicated rows, a zero row, simplex -- each through the one-set operations and every ordered pair of
                   them through the pair operations, the extended list (region_diff against Regions, Region.intersect,
                   is_subset of a Region, extreme at d <= 3, projection at d >= 2) included;
  g33_objects      40 random triples (seed 11, d = 1..4) through the operations of scripts/soak_objects_cpu.py.

The reference is imported in place and only run; the files hold the arrays, booleans and exception class names it gave,
as JSON in which floats round-trip exactly.  np.random is seeded before every operation (the reference's `==` on tiny
pieces samples volumes with the global generator), the gzip header carries no time: two runs give the same bytes.

    REF_POLYTOPE=<checkout of tulip-control/polytope> PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_edges.py [--to DIR] [1 2 3 4 objects]
(--to DIR: write there instead of tests/golden, to compare two runs)
"""
import logging
import os
import sys
import warnings

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.environ["REF_POLYTOPE"])
import polytope as ref  # noqa: E402  (the reference)
import edge_cases as E  # noqa: E402

logging.disable(logging.CRITICAL)
warnings.simplefilter("ignore")   # (inf - inf in the reference's sampled volumes and box comparisons of open sets)


OUT = HERE
if "--to" in sys.argv:
    OUT = sys.argv[sys.argv.index("--to") + 1]
    del sys.argv[sys.argv.index("--to"):sys.argv.index("--to") + 2]


def record_edges(d):
    rec = E.Reference.recorder(os.path.join(OUT, os.path.basename(E.EDGE_FIXTURE % d)), ref, os.path.basename(__file__), [str(d)])
    items, cases = E.edge_cases(d)
    nexc = 0
    for what, fn, cmp, operands in cases:
        for names in operands:
            out = rec.outcome(E.edge_key(d, what, names), lambda mod: E.edge_outcome(mod, items, names, fn))
            nexc += out[0] == "exc"
    rec.save()
    print("%s: %d outcomes, %d of them exceptions, %d bytes" % (
        os.path.basename(rec.path), len(rec.store), nexc, os.path.getsize(rec.path)))


def record_objects():
    rec = E.Reference.recorder(os.path.join(OUT, os.path.basename(E.OBJECT_FIXTURE)), ref, os.path.basename(__file__), E.OBJECT_ARGS)
    for trial, d, kinds, data in E.triples(int(E.OBJECT_ARGS[0]), int(E.OBJECT_ARGS[1])):
        for what, fn, cmp in E.object_ops(d):
            rec.outcome(E.object_key(trial, what), lambda mod: E.object_outcome(mod, data, trial, fn))
    rec.save()
    print("%s: %d outcomes, %d bytes" % (os.path.basename(rec.path), len(rec.store), os.path.getsize(rec.path)))


if __name__ == "__main__":
    for what in sys.argv[1:] or [str(d) for d in E.EDGE_DIMS] + ["objects"]:
        record_objects() if what == "objects" else record_edges(int(what))
