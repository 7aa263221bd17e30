"""What scripts/soak_edges_cpu.py, scripts/soak_objects_cpu.py, tests/golden/make_golden_edges.py, tests/test_edge_objects.py
(CPU) and tests/test_edge_objects_gpu.py share: the object layer (Polytope / Region) held to what THE REFERENCE ITSELF
returned, on sets that are not nice bounded polytopes and on random triples.

menu()            14 sets per dimension: empty, box, shifted / touching / apart / tiny boxes, half-space, slab, flat,
                  infeasible, open cone, duplicated rows, a zero row, simplex;
menu_extended()   those plus box_rows (the box under 32 redundant rows: more than 32 rows in all, beyond the listed-pair
                  kernels' cells and into the 33..64-row tiles), box_scaled (a box whose rows are scaled by 1e-3 .. 1e3:
                  the constructor's normalisation) and box_far (the box translated by 100).  No width, gap or radius of
                  the three is within a factor 100 of abs_tol = 1e-7: the nearest are 0 (rows that coincide) and 1e-3;
ops1(), ops2()    the light operations on one set / on an ordered pair;  ops1_more(), ops2_more() the extended list
                  (region_diff against one- and two-cell Regions, Region.intersect, is_subset of a Region, extreme,
                  projection);
same, eqb, eqbox, eqnum, eqdim, eqverts    the comparison rules: pieces in order with rows to 1e-9, booleans exact, boxes
                  to 1e-9 with equal_nan, numbers to 1e-9, vertices as a set to 1e-9; mismatch() adds the rule for
                  exceptions (the class, exactly);
Reference         the reference side: the reference itself (recording what it returned) or a recording of it;
triples(), object_ops()   the random triples of soak_objects_cpu.py and their operations;
edge_differences(), object_differences()  the package on every recorded key, on the backend that `backend()` sets.
Helpers only: no tests here."""
import contextlib
import gzip
import itertools
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
EDGE_DIMS = (1, 2, 3, 4)
EDGE_FIXTURE = os.path.join(GOLDEN, "g32_edges_d%d.json.gz")        # one per dimension
OBJECT_FIXTURE = os.path.join(GOLDEN, "g33_objects.json.gz")
OBJECT_ARGS = ["40", "11"]                                           # trials, seed of g33
OLD_OBJECT_FIXTURE = os.path.join(GOLDEN, "g26_objects_cpu.json.gz")
OLD_OBJECT_ARGS = ["6", "3"]
NEW_ITEMS = ("box_rows", "box_scaled", "box_far")
TOL = 1e-9


@contextlib.contextmanager
def backend(name):
    """solvers.default_solver = name for the block; the solver found is put back."""
    from polytope_amd import solvers
    old = solvers.default_solver
    solvers.default_solver = name
    try:
        yield
    finally:
        solvers.default_solver = old


# ------------------------------------------------------------------------------------------------ recorded values
class Piece:
    """A recorded piece of a result: what `same` reads of a Polytope."""
    def __init__(self, A, b):
        self.A, self.b = A, b


def pieces(X):
    if isinstance(X, (list, tuple)):   # recorded
        return list(X)
    if hasattr(X, "list_poly"):        # a Region, the package's or the reference's
        return list(X.list_poly)
    return [X] if X.A.size else []


def _arr(a):
    a = np.asarray(a)
    return {"array": a.tolist(), "shape": list(a.shape), "dtype": str(a.dtype)}


def encode(v):
    """A result of an operation as JSON (floats round-trip exactly)."""
    if hasattr(v, "list_poly") or (hasattr(v, "A") and hasattr(v, "b")):
        return {"pieces": [[_arr(p.A), _arr(p.b)] for p in pieces(v)]}
    if isinstance(v, np.ndarray):
        return _arr(v)
    if isinstance(v, (tuple, list)):
        return [encode(u) for u in v]
    if isinstance(v, (bool, np.bool_)):
        return bool(v)
    if isinstance(v, (int, np.integer)):
        return int(v)
    if isinstance(v, (float, np.floating)):
        return float(v)
    if v is None:
        return None
    raise TypeError("cannot record a %s" % type(v).__name__)


def decode(v):
    if isinstance(v, dict):
        if "pieces" in v:
            return [Piece(decode(A), decode(b)) for A, b in v["pieces"]]
        return np.array(v["array"], dtype=v["dtype"]).reshape(v["shape"])
    if isinstance(v, list):
        return tuple(decode(u) for u in v)
    return v


class Reference:
    """The reference side of a comparison: the reference itself (recording what it returned with --record FILE), or the
    outcomes such a file stored (--against FILE).  Takes its option out of argv.  Reference.replay(path) and
    Reference.recorder(path, module, script, args) are the same two without a command line."""

    def __init__(self, argv):
        self.mode, self.path, self.store, self.ref = None, None, {}, None
        self.script = os.path.basename(argv[0]) if argv else ""
        for opt in ("--record", "--against"):
            if opt in argv:
                i = argv.index(opt)
                self.mode, self.path = opt[2:], argv[i + 1]
                del argv[i:i + 2]
        self.args = argv[1:]
        if self.mode == "against":
            self._load()
            if self.recorded_args != self.args:
                raise SystemExit("%s was recorded with the arguments %s, not %s" % (self.path, self.recorded_args, self.args))
        else:
            if os.environ.get("POLYTOPE_REFERENCE"):
                sys.path.insert(0, os.environ["POLYTOPE_REFERENCE"])
            import polytope
            self.ref = polytope

    def _load(self):
        with gzip.open(self.path, "rt") as f:
            rec = json.load(f)
        self.recorded_args, self.store = rec["args"], rec["outcomes"]

    @classmethod
    def replay(cls, path):
        self = cls.__new__(cls)
        self.mode, self.path, self.ref, self.script, self.args = "against", path, None, "", None
        self._load()
        return self

    @classmethod
    def recorder(cls, path, module, script, args):
        self = cls.__new__(cls)
        self.mode, self.path, self.ref, self.script, self.args, self.store = "record", path, module, script, list(args), {}
        return self

    def keys(self):
        return list(self.store)

    def outcome(self, key, run):
        """run(module) -> ("ok", value) or ("exc", exception class name)"""
        if self.mode == "against":
            kind, v = self.store[key]
            return (kind, decode(v)) if kind == "ok" else (kind, v)
        out = run(self.ref)
        if self.mode == "record":
            self.store[key] = [out[0], encode(out[1]) if out[0] == "ok" else out[1]]
        return out

    def save(self):
        if self.mode == "record":
            with gzip.GzipFile(self.path, "wb", mtime=0) as f:
                f.write(json.dumps({"script": self.script, "args": self.args, "outcomes": self.store}, sort_keys=True).encode())


# ------------------------------------------------------------------------------------------------ comparison rules
def same(X, Y, what, tol=TOL):
    a, b = pieces(X), pieces(Y)
    if len(a) != len(b):
        return "%s: %d pieces against %d" % (what, len(a), len(b))
    for k, (p, q) in enumerate(zip(a, b)):
        if p.A.shape != q.A.shape:
            return "%s: piece %d has %s rows against %s" % (what, k, p.A.shape, q.A.shape)
        if not (np.allclose(p.A, q.A, rtol=0, atol=tol) and np.allclose(p.b, q.b, rtol=0, atol=tol)):
            return "%s: piece %d rows differ by %.2e" % (what, k, max(np.abs(p.A - q.A).max(), np.abs(p.b - q.b).max()))
    return None


def same_unordered(X, Y, what, tol=TOL):
    """`same` without the order of the pieces: each piece of X is some piece of Y not used before (rows in order, to tol)."""
    a, b = pieces(X), pieces(Y)
    if len(a) != len(b):
        return "%s: %d pieces against %d" % (what, len(a), len(b))
    left = list(b)
    for k, p in enumerate(a):
        hit = next((q for q in left if same([p], [q], what, tol) is None), None)
        if hit is None:
            return "%s: piece %d is none of the other side's" % (what, k)
        left.remove(hit)
    return None


def eqb(x, y, w):
    return None if bool(x) == bool(y) else "%s: %s against %s" % (w, x, y)


def eqbox(x, y, w):
    ok = all(np.allclose(np.asarray(u, float), np.asarray(v, float), rtol=0, atol=TOL, equal_nan=True) for u, v in zip(x, y))
    return None if ok else "%s: %s against %s" % (w, [np.ravel(u) for u in x], [np.ravel(v) for v in y])


def eqnum(x, y, w):
    return None if (x is None and y is None) or abs(float(x) - float(y)) <= TOL else "%s: %r against %r" % (w, x, y)


def eqdim(x, y, w):
    return None if x == y else w + ": %r against %r" % (x, y)


def eqverts(x, y, w):
    """Vertices as a set: the same number, and each within 1e-9 of one of the other side's (both None: no vertices)."""
    if x is None or y is None:
        return None if x is None and y is None else "%s: %s against %s" % (w, "None" if x is None else "vertices", "None" if y is None else "vertices")
    x, y = np.asarray(x, float), np.asarray(y, float)
    if x.shape != y.shape:
        return "%s: %s vertices against %s" % (w, x.shape, y.shape)
    gap = np.abs(x[:, None, :] - y[None, :, :]).max(axis=2)
    worst = max(gap.min(axis=1).max(), gap.min(axis=0).max()) if x.size else 0.0
    return None if worst <= TOL else "%s: vertices differ by %.2e" % (w, worst)


def eqverts_loose(x, y, w):
    """soak_objects_cpu.py's rule for extreme (g26 was recorded and is replayed under it)."""
    ok = (x is None and y is None) or (x is not None and y is not None and x.shape == y.shape
                                       and np.allclose(np.sort(x, 0), np.sort(y, 0), atol=1e-7))
    return None if ok else w + ": vertices differ"


def mismatch(want, got, cmp, what):
    """None, or how the outcome `got` differs from the recorded `want`: ok against raised, the exception class, or cmp."""
    if want[0] != got[0] or (want[0] == "exc" and want[1] != got[1]):
        return "reference %s, package %s" % (want if want[0] == "exc" else "ok", got if got[0] == "exc" else "ok")
    if want[0] == "ok":
        try:
            return cmp(want[1], got[1], what)
        except Exception as e:
            return "comparison failed: %r" % (e,)
    return None


# ------------------------------------------------------------------------------------------------ the edge menu
def menu(d):
    I = np.eye(d)
    box = (np.vstack([I, -I]), np.r_[np.ones(d), np.zeros(d)])
    items = {
        "empty": (np.zeros((0, d)), np.zeros(0)),
        "box": box,
        "box_shift": (box[0], box[1] + box[0] @ (0.5 * np.ones(d))),
        "box_touch": (box[0], box[1] + box[0] @ np.r_[1.0, np.zeros(d - 1)]),
        "box_apart": (box[0], box[1] + box[0] @ (3.0 * np.ones(d))),
        "tiny": (box[0], 1e-3 * box[1]),
        "halfspace": (I[:1], np.array([0.5])),
        "slab": (np.vstack([I[:1], -I[:1]]), np.array([0.7, -0.3])),
        "flat": (np.vstack([box[0], I[:1], -I[:1]]), np.r_[box[1], 0.5, -0.5]),
        "infeasible": (np.vstack([box[0], I[:1]]), np.r_[box[1], -1.0]),
        "cone": (-I, np.zeros(d)),
        "dup_rows": (np.vstack([box[0], box[0][:2]]), np.r_[box[1], box[1][:2] + [0.0, 0.2]]),
        "zero_row": (np.vstack([box[0], np.zeros((1, d))]), np.r_[box[1], 1.0]),
        "simplex": (np.vstack([-I, np.ones((1, d)) / np.sqrt(d)]), np.r_[np.zeros(d), 0.6]),
    }
    return items


def menu_extended(d):
    items = menu(d)
    A, b = items["box"]
    rng = np.random.default_rng(3200 + d)
    G = rng.standard_normal((32, d))
    G /= np.linalg.norm(G, axis=1, keepdims=True)
    # redundant by 0.3 .. 0.8: each row's largest value over the box [0, 1]^d is the sum of its positive entries
    items["box_rows"] = (np.vstack([A, G]), np.r_[b, np.maximum(G, 0).sum(axis=1) + rng.uniform(0.3, 0.8, 32)])
    s = np.logspace(-3, 3, 2 * d)
    items["box_scaled"] = (A * s[:, None], (b + A @ (-0.25 * np.ones(d))) * s)     # [-0.25, 0.75]^d
    items["box_far"] = (A, b + A @ (100.0 * np.ones(d)))                            # [100, 101]^d
    return items


def ops1(d):
    return [
        ("reduce", lambda m, P: m.reduce(P), same),
        ("cheby_ball", lambda m, P: m.cheby_ball(P)[0], eqnum),
        ("is_fulldim", lambda m, P: m.is_fulldim(P), eqb),
        ("is_empty", lambda m, P: m.is_empty(P), eqb),
        ("bounding_box", lambda m, P: P.bounding_box, eqbox),
        ("Region([P])", lambda m, P: m.Region([P]), same),
        ("Region([P, empty])", lambda m, P: m.Region([P, m.Polytope()]), same),
        ("Region bounding_box", lambda m, P: m.Region([P, P.copy()]).bounding_box, eqbox),
        ("copy ==", lambda m, P: P == P.copy(), eqb),
        ("contains centre", lambda m, P: (0.5 * np.ones((d, 1))) in P if P.A.size else False, eqb),
        ("dim", lambda m, P: P.dim, eqdim),
    ]


def ops2(d):
    ops = [
        ("intersect", lambda m, P, Q: P.intersect(Q), same),
        ("is_adjacent", lambda m, P, Q: m.is_adjacent(P, Q), eqb),
        ("is_subset", lambda m, P, Q: m.is_subset(P, Q), eqb),
        ("mldivide", lambda m, P, Q: m.mldivide(P, Q), same),
        ("union", lambda m, P, Q: m.union(P, Q), same),
        ("envelope", lambda m, P, Q: m.envelope(m.Region([P, Q])), same),
        ("is_convex", lambda m, P, Q: m.is_convex(m.Region([P, Q]))[0], eqb),
        ("<=", lambda m, P, Q: P <= Q, eqb),
    ]
    if d <= 2:
        ops.append(("union(check_convex)", lambda m, P, Q: m.union(P, Q, check_convex=True), same))
    return ops


def ops1_more(d):
    ops = []
    if d <= 3:
        ops.append(("extreme", lambda m, P: m.extreme(P), eqverts))
    if d >= 2:
        ops.append(("projection(P, [1])", lambda m, P: m.polytope.projection(P, [1]), same))
    return ops


def ops2_more(d):
    items = menu(d)
    fresh = lambda m, n: m.Polytope(items[n][0].copy(), items[n][1].copy())   # noqa: E731
    return [
        ("region_diff(P, Region([Q]))", lambda m, P, Q: m.polytope.region_diff(P, m.Region([Q])), same),
        ("region_diff(P, Region([Q, box_shift]))", lambda m, P, Q: m.polytope.region_diff(P, m.Region([Q, fresh(m, "box_shift")])), same),
        ("Region([P, Q]).intersect(box_shift)", lambda m, P, Q: m.Region([P, Q]).intersect(fresh(m, "box_shift")), same),
        ("is_subset(Region([P, Q]), box)", lambda m, P, Q: m.is_subset(m.Region([P, Q]), fresh(m, "box")), eqb),
    ]


def edge_key(d, what, names):
    return "%d %s %s" % (d, what, "/".join(names))


def edge_outcome(mod, items, names, fn):
    """("ok", value) or ("exc", class name) of fn on fresh copies of the named items, np.random seeded (the reference's `==`
    on tiny pieces samples volumes with the global generator)."""
    args = [mod.Polytope(items[n][0].copy(), items[n][1].copy()) for n in names]
    try:
        np.random.seed(0)
        return ("ok", fn(mod, *args))
    except Exception as e:
        return ("exc", type(e).__name__)


def edge_cases(d, extended=True):
    """[(what, fn, cmp, [names of the operands, ...]), ...] for one dimension: every item through the one-set operations,
    every ordered pair through the pair operations; `extended` adds the three new items and the extended operations."""
    items = menu_extended(d) if extended else menu(d)
    o1 = ops1(d) + (ops1_more(d) if extended else [])
    o2 = ops2(d) + (ops2_more(d) if extended else [])
    singles = [[n] for n in items]
    pairs = [[n1, n2] for n1, n2 in itertools.product(items, items)]
    return items, [(what, fn, cmp, singles) for what, fn, cmp in o1] + [(what, fn, cmp, pairs) for what, fn, cmp in o2]


# ------------------------------------------------------------------------------------------------ random triples
def rand_poly(rng, d, kind):
    if kind == "box":
        lo = rng.uniform(-1, 0.5, d)
        hi = lo + rng.uniform(0.3, 1.5, d)
        return np.vstack([np.eye(d), -np.eye(d)]), np.hstack([hi, -lo])
    m = int(rng.integers(d + 1, 4 * d + 3))
    A = rng.standard_normal((m, d))
    A /= np.linalg.norm(A, axis=1, keepdims=True)
    c = rng.uniform(-0.4, 0.4, d)
    b = A @ c + rng.uniform(0.3, 1.0, m)
    if kind == "boxed":
        A = np.vstack([A, np.eye(d), -np.eye(d)])
        b = np.hstack([b, np.full(d, 1.5), np.full(d, 1.5)])
    return A, b


def triples(trials, seed):
    """(trial, d, kinds, [(A, b)] * 3) per trial; every fourth a hyperplane split of the first polytope (touching pieces,
    convex union)."""
    rng = np.random.default_rng(seed)
    for trial in range(trials):
        d = int(rng.choice([1, 2, 2, 3, 3, 4]))
        kinds = [str(rng.choice(["box", "boxed", "boxed", "free"])) for _ in range(3)]
        data = [rand_poly(rng, d, k) for k in kinds]
        if trial % 4 == 0:
            A0, b0 = data[0]
            n = rng.standard_normal(d); n /= np.linalg.norm(n)
            off = float(n @ rng.uniform(-0.2, 0.2, d))
            data[1] = (np.vstack([A0, n]), np.hstack([b0, off]))
            data[2] = (np.vstack([A0, -n]), np.hstack([b0, -off]))
        yield trial, d, kinds, data


def object_ops(d):
    """[(what, fn(module, [P0, P1, P2]), cmp)] of a triple in dimension d."""
    eqbox = lambda x, y, w: None if all(np.allclose(u, v, rtol=0, atol=TOL, equal_nan=True) for u, v in zip(x, y)) else w + ": boxes differ"  # noqa: E731  (the script's own line)
    heavy = d <= 2   # (the reference's union(check_convex) chains cost minutes per call from d = 3 on: 2 ms per LP)
    ops = [("reduce", lambda m, P: m.reduce(P[0]), same),
           ("intersect", lambda m, P: P[0].intersect(P[1]), same)]
    if heavy:
        ops.append(("union(check_convex)", lambda m, P: m.union(P[1], P[2], check_convex=True), same))
    ops += [("union", lambda m, P: m.union(P[0], P[1], check_convex=False), same),
            ("mldivide", lambda m, P: m.mldivide(P[0], P[1]), same),
            ("mldivide(P, Region)", lambda m, P: m.mldivide(P[0], m.Region([P[1], P[2]])), same)]
    if heavy:
        ops.append(("mldivide(Region, P)", lambda m, P: m.mldivide(m.Region([P[0], P[1]]), P[2]), same))
    ops += [("envelope", lambda m, P: m.envelope(m.Region([P[1], P[2]])), same),
            ("is_convex", lambda m, P: m.is_convex(m.Region([P[1], P[2]]))[0], eqb),
            ("is_adjacent", lambda m, P: m.is_adjacent(P[1], P[2]), eqb),
            ("is_adjacent(overlap)", lambda m, P: m.is_adjacent(P[0], P[1], overlap=True), eqb),
            ("is_subset", lambda m, P: m.is_subset(P[1], P[0]), eqb)]
    if heavy:
        ops.append(("is_subset(Region, P)", lambda m, P: m.is_subset(m.Region([P[1], P[2]]), P[0]), eqb))
    ops += [("bounding_box", lambda m, P: P[1].bounding_box, eqbox),
            ("Region.bounding_box", lambda m, P: m.Region([P[0], P[1]]).bounding_box, eqbox),
            ("is_fulldim", lambda m, P: m.is_fulldim(P[0].intersect(P[2])), eqb)]
    if heavy:
        ops += [("Region.intersect", lambda m, P: m.Region([P[0], P[1]]).intersect(P[2]), same),
                ("Region.diff", lambda m, P: m.Region([P[1], P[2]]).diff(P[0]), same)]
    ops.append(("cheby_ball", lambda m, P: m.cheby_ball(P[0])[0], lambda x, y, w: None if abs(x - y) <= TOL else "%s: %r against %r" % (w, x, y)))
    if d <= 3:
        ops.append(("extreme", lambda m, P: m.extreme(P[1]), eqverts_loose))
    return ops


def object_key(trial, what):
    return "%d %s" % (trial, what)


def object_outcome(mod, data, trial, fn):
    P = [mod.Polytope(A.copy(), b.copy()) for A, b in data]
    try:
        np.random.seed(trial)
        return ("ok", fn(mod, P))
    except Exception as e:   # the same exception class on both sides is parity too
        return ("exc", type(e).__name__)


# ------------------------------------------------------------------------------------------------ replay
def edge_differences(reference, mod, d, extended=True, only=None, rules=None):
    """The package `mod` on every key of dimension d (or of the operation `only`) against `reference`
    -> (number of keys, {key: how it differs}).  `rules` ({key: cmp}): these keys alone, each under the rule given."""
    items, cases = edge_cases(d, extended)
    n, diffs = 0, {}
    for what, fn, cmp, operands in cases:
        if only is not None and what != only:
            continue
        for names in operands:
            key = edge_key(d, what, names)
            if rules is not None and key not in rules:
                continue
            n += 1
            err = mismatch(reference.outcome(key, None), edge_outcome(mod, items, names, fn), (rules or {}).get(key, cmp), what)
            if err:
                diffs[key] = err
    return n, diffs


def object_differences(reference, mod, trials, seed, only=None, rules=None):
    """The same for the random triples (`only`: one trial) -> (number of keys, {key: how it differs})."""
    n, diffs = 0, {}
    for trial, d, kinds, data in triples(trials, seed):
        if only is not None and trial != only:
            continue
        for what, fn, cmp in object_ops(d):
            key = object_key(trial, what)
            if rules is not None and key not in rules:
                continue
            n += 1
            err = mismatch(reference.outcome(key, None), object_outcome(mod, data, trial, fn), (rules or {}).get(key, cmp), what)
            if err:
                diffs[key] = err
    return n, diffs
