#!/usr/bin/env python3
"""CPU: EDGE inputs through the host layer against the reference itself (both on the scipy backend; build container only, the
reference is imported in place): empty polytopes, half-spaces, slabs, flat (lower-dimensional) sets, open cones, tiny boxes,
duplicated and zero rows, one-member and empty Regions -- every pair of a menu through the light operations; results (pieces in
order, rows 1e-9, booleans, boxes) or the exception CLASS must agree.
    python scripts/soak_edges_cpu.py [--record FILE | --against FILE] [d ...]
The reference, --record and --against: as in scripts/soak_objects_cpu.py."""
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
from edge_cases import Reference, edge_cases, edge_key, edge_outcome, mismatch  # noqa: E402  (the menu, the operations, the rules)


def main():
    reference = Reference(sys.argv)
    dims = [int(a) for a in sys.argv[1:]] or [1, 2, 3]
    bad = nops = 0
    t0 = time.time()
    for d in dims:
        items, cases = edge_cases(d, extended=False)

        def run(what, fn, cmp, names):
            nonlocal bad, nops
            nops += 1
            key = edge_key(d, what, names)
            err = mismatch(reference.outcome(key, lambda mod: edge_outcome(mod, items, names, fn)),
                           edge_outcome(mine, items, names, fn), cmp, what)
            if err:
                bad += 1
                print("d=%d %-20s %-24s %s" % (d, what, "/".join(names), err), flush=True)

        for arity in (1, 2):   # each item through its operations, then each pair
            group = [c for c in cases if len(c[3][0]) == arity]
            for names in group[0][3]:
                for what, fn, cmp, _ in group:
                    run(what, fn, cmp, names)
        print("d=%d done: %d operations so far, %d differences, %.0f s" % (d, nops, bad, time.time() - t0), flush=True)
    reference.save()
    print("EDGE SOAK (cpu, scipy backend on both sides) %s: %d operations, %d differences" % ("FAILED" if bad else "OK", nops, bad))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
