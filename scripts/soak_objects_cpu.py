#!/usr/bin/env python3
"""CPU soak of the HOST layer (polytope_amd/polytope.py, prop2partition.py) against the reference itself, both on the scipy
backend, in the build container only (/root/reference is imported in place; nothing of it is copied): random and structured
polytope pairs / small regions in d = 1..4 through reduce, intersect, union(check_convex), mldivide, envelope, is_convex,
is_adjacent, is_subset, ==, bounding_box, extreme, Region.intersect, Region diff, find_adjacent_regions -- same pieces in the
same order, rows within 1e-9, booleans equal.    python scripts/soak_objects_cpu.py [--record FILE | --against FILE] [trials] [seed]

The reference is the package `polytope` as Python finds it, or the checkout that POLYTOPE_REFERENCE names.
--record FILE also stores what the reference returned (gzip'd JSON); --against FILE compares with such a file instead
of the reference, which then need not be there (tests/test_against_reference.py)."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.dont_write_bytecode = True
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import logging  # noqa: E402
logging.disable(logging.CRITICAL)
import polytope_amd as mine  # noqa: E402
assert mine.solvers.default_solver != "hip"
from edge_cases import Reference, object_key, object_ops, object_outcome, triples  # noqa: E402  (the generator, the operations, the rules)


def main():
    reference = Reference(sys.argv)
    trials = int(sys.argv[1]) if len(sys.argv) > 1 else 200
    seed = int(sys.argv[2]) if len(sys.argv) > 2 else 1
    bad = 0
    t0 = time.time()
    nops = 0
    for trial, d, kinds, data in triples(trials, seed):
        errs = []
        only = os.environ.get("SOAK_ONLY")
        if only is not None and int(only) != trial:
            continue

        def both(fn, what, cmp):
            nonlocal nops
            nops += 1

            def run(mod):
                t1 = time.time()
                o = object_outcome(mod, data, trial, fn)
                if only is not None:
                    print("   %-22s %-10s %.2f s" % (what, mod.__name__, time.time() - t1), flush=True)
                return o
            out = [reference.outcome(object_key(trial, what), run), run(mine)]
            if out[0][0] != out[1][0]:
                errs.append("%s: reference %s, package %s" % (what, out[0], out[1]))
            elif out[0][0] == "exc":
                if out[0][1] != out[1][1]:
                    errs.append("%s: exceptions %s / %s" % (what, out[0][1], out[1][1]))
            else:
                e = cmp(out[0][1], out[1][1], what)
                if e:
                    errs.append(e)

        for what, fn, cmp in object_ops(d):
            both(fn, what, cmp)
        if errs:
            bad += 1
            print("trial %d  d %d %s:" % (trial, d, kinds), "; ".join(errs[:4]), flush=True)
        elif os.environ.get("SOAK_VERBOSE"):
            print("trial %d  d %d %s ok  %.0f s" % (trial, d, kinds, time.time() - t0), flush=True)
    reference.save()
    print("OBJECT SOAK (cpu, scipy backend on both sides) %s: %d trials, %d operations, %d trials with a difference, %.0f s" % (
        "FAILED" if bad else "OK", trials, nops, bad, time.time() - t0), flush=True)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
