"""CPU: the host layer against what THE REFERENCE ITSELF returned on the same operations (both on the scipy backend),
recorded by the soak scripts with --record into tests/golden/g25_edges_cpu.json.gz and g26_objects_cpu.json.gz; nothing
of the reference is copied.  The long forms, against the reference itself, are scripts/soak_edges_cpu.py and
scripts/soak_objects_cpu.py."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def _run(script, *args, timeout=900):
    env = dict(os.environ, PYTHONDONTWRITEBYTECODE="1")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", script)] + list(args), capture_output=True, text=True,
                         timeout=timeout, env=env, cwd=ROOT)
    return out.returncode, out.stdout


def test_edge_menu_against_the_reference():
    """empty / half-space / slab / flat / infeasible / cone / tiny / duplicated and zero rows, every pair of the menu through 19
    light operations at d = 1 (scripts/soak_edges_cpu.py 1 2 3: 5 558 operations): same pieces in the same order (rows 1e-9), same booleans and boxes, same exception classes."""
    rc, out = _run("soak_edges_cpu.py", "--against", os.path.join(GOLDEN, "g25_edges_cpu.json.gz"), "1")
    assert rc == 0 and "EDGE SOAK (cpu, scipy backend on both sides) OK" in out, out[-2000:]


def test_random_objects_against_the_reference():
    """random polytope triples in d = 1..4 through reduce / intersect / union / mldivide / envelope / is_convex / is_adjacent /
    is_subset / bounding_box / extreme (+ the Region forms and union(check_convex) at d <= 2): 6 trials."""
    rc, out = _run("soak_objects_cpu.py", "--against", os.path.join(GOLDEN, "g26_objects_cpu.json.gz"), "6", "3")
    assert rc == 0 and "OBJECT SOAK (cpu, scipy backend on both sides) OK" in out, out[-2000:]
