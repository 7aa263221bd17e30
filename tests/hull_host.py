"""Host build of polytope_amd/csrc/plp_hull_enum.hpp (tests/cabi/hull_enum_host.cpp, g++ -ffp-contract=off) and what
tests/test_hull_host.py (CPU: the sequential rule against the reference's quickhull()) and tests/test_hull_gpu.py (the
kernel against the host build bit for bit, the public hull_batch against the fixture) share: the fixture
tests/golden/g30_hull.npz, the comparison rule and the cap on cases left out of it."""
import ctypes as C
import os

import numpy as np

import host_build as hb
from host_build import ROOT, keep_word, same_bits, ptr as _p, upper_bound as fmax_for  # noqa: F401

SRC = os.path.join(ROOT, "tests", "cabi", "hull_enum_host.cpp")

HS_OK, HS_OVERFLOW, HS_FLAT = 0, 1, 2
SIDE_TOL = 1e-9
# what the reference's quickhull() did with a case (the fixture's `ref_kind`)
REF_ROWS, REF_EMPTY, REF_RAISED = 0, 1, 2
# the comparison with the fixture, as sets, in the distance |dA|_inf + |db| / scale between rows of unit normal: the
# reference's rows collapsed at COLLAPSE (its simplicial facets repeat a degenerate face), then equal counts and every
# reference row within MATCH max(1, |b| / scale) of one of ours
COLLAPSE, MATCH = 1e-7, 1e-6
# cases left out of the comparison (`pinned` false in the fixture, with a reason code): at most this share of any family
UNPINNED_CAP = 0.02


def build(tmpdir, as_path=False):
    """Compiles the host build into tmpdir -> the loaded library, or (as_path) the path of the shared object."""
    out = hb.build(SRC, "libhull_enum_host.so", tmpdir)
    return out if as_path else load(out)


def build_program(tmpdir):
    """The stand-alone program (-DHULL_HOST_MAIN) under -fsanitize=address,undefined -> its path."""
    return hb.build_program(SRC, "HULL_HOST_MAIN", "hull_enum_host_san", tmpdir)


def load(out):
    L = C.CDLL(out)
    L.hull_enum_host.restype = C.c_int
    L.hull_enum_host.argtypes = [C.c_longlong, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p,
                                 C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    return L


def run(L, X, n=None, keep=None, f_max=None, basis=True):
    """plp_hull_batch on the host -> dict(A[B, f_max, d], b[B, f_max], on uint64[B, f_max], count[B], basis or None,
    status[B])."""
    X = np.ascontiguousarray(X, dtype=np.float64)
    B, n_max, d = X.shape
    n = None if n is None else np.ascontiguousarray(n, dtype=np.int32)
    keep = None if keep is None else np.ascontiguousarray(keep, dtype=np.uint64)
    f_max = fmax_for(d, n_max) if f_max is None else f_max
    A, b, on = np.empty((B, f_max, d)), np.empty((B, f_max)), np.empty((B, f_max), np.uint64)
    count, status = np.empty(B, np.int32), np.empty(B, np.int32)
    bas = np.empty((B, f_max, d), np.int32) if basis else None
    rc = L.hull_enum_host(B, n_max, d, _p(X), _p(n), _p(keep), f_max, _p(A), _p(b), _p(on), _p(count), _p(bas), _p(status))
    assert rc == 0
    return dict(A=A, b=b, on=on, count=count, basis=bas, status=status)


def bits(word):
    """a uint64 word -> the set of its bit positions."""
    return {i for i in range(64) if (int(word) >> i) & 1}


def same_result(got, want, basis=True):
    """Two results of the rule: status, count, on, basis identical, A and b bit for bit -> None or what differs."""
    for k in ("status", "count", "on") + (("basis",) if basis else ()):
        if not np.array_equal(np.asarray(got[k]), np.asarray(want[k])):
            return "%s differs at %s" % (k, np.argwhere(np.asarray(got[k]) != np.asarray(want[k]))[:4].tolist())
    for k in ("A", "b"):
        if not same_bits(got[k], want[k]):
            return "%s differs in its bits" % k
    return None


# ------------------------------------------------------------------------------------------------ the fixture
def fixture():
    """tests/golden/g30_hull.npz (tests/golden/make_golden_hull.py) -> a list of dicts: index, family, d, scale, X (the
    points), A, b (the reference's raw rows, empty unless ref_kind is REF_ROWS), ref_kind, pinned, reason."""
    z = np.load(os.path.join(ROOT, "tests", "golden", "g30_hull.npz"), allow_pickle=False)
    z = {k: z[k] for k in z.files}
    fams = [str(s) for s in z["families"]]
    out = []
    for c in range(len(z["family"])):
        d = int(z["d"][c])
        lo, hi = z["row_off"][c], z["row_off"][c + 1]
        out.append(dict(index=c, family=fams[z["family"][c]], d=d, scale=float(z["scale"][c]),
                        X=z["X"][z["x_off"][c]:z["x_off"][c + 1]].reshape(-1, d),
                        A=z["A"][z["a_off"][c]:z["a_off"][c + 1]].reshape(hi - lo, d), b=z["b"][lo:hi],
                        ref_kind=int(z["ref_kind"][c]), pinned=bool(z["pinned"][c]), reason=int(z["reason"][c])))
    return out


def pack(cases, d):
    """The cases of dimension d as one packed batch -> (indices into `cases`, X[B, n_max, d], n[B]); padding is zero."""
    sel = [i for i, c in enumerate(cases) if c["d"] == d]
    n = np.array([cases[i]["X"].shape[0] for i in sel], np.int32)
    X = np.zeros((len(sel), int(n.max()), d))
    for k, i in enumerate(sel):
        X[k, :n[k]] = cases[i]["X"]
    return sel, X, n


def ref_rows(case):
    """The reference's rows with unit normals, its repeats of one face taken out (greedy, COLLAPSE) -> (A, b)."""
    nrm = np.linalg.norm(case["A"], axis=1)
    A, b = case["A"] / nrm[:, None], case["b"] / nrm
    keepA, keepb = [], []
    for a, beta in zip(A, b):
        if not any(np.max(np.abs(a - w)) + abs(beta - v) / case["scale"] <= COLLAPSE for w, v in zip(keepA, keepb)):
            keepA.append(a)
            keepb.append(beta)
    return np.array(keepA).reshape(-1, case["d"]), np.array(keepb)


def compare(case, A, b, count, status):
    """One case against the fixture -> None, or what is wrong (a string).  A[count, d], b[count]: our rows."""
    kind = case["ref_kind"]
    if kind == REF_RAISED:
        return "the reference raised"
    if (kind == REF_EMPTY) != (status == HS_FLAT):
        return "status %d where the reference has kind %d" % (status, kind)
    if kind == REF_EMPTY:
        return None if count == 0 else "%d rows of a flat set" % count
    if status != HS_OK:
        return "status %d" % status
    RA, Rb = ref_rows(case)
    if len(Rb) != count:
        return "%d rows for the reference's %d (%d raw)" % (count, len(Rb), len(case["b"]))
    worst = 0.0
    for a, beta in zip(RA, Rb):
        dist = np.min(np.max(np.abs(A[:count] - a), axis=1) + np.abs(b[:count] - beta) / case["scale"])
        worst = max(worst, dist / max(1.0, abs(beta) / case["scale"]))
    if worst > MATCH:
        return "rows off by %.1e" % worst
    return None


def check_cases(cases, results, what):
    """results[i] = (A, b, count, status) of case i.  Pinned cases must compare clean; unpinned ones are listed with their
    reason, and their number is held to UNPINNED_CAP of their family.  -> the number of unpinned cases."""
    wrong, unpinned, per_family = [], {}, {}
    for c, (A, b, count, status) in zip(cases, results):
        per_family[c["family"]] = per_family.get(c["family"], 0) + 1
        msg = compare(c, A, b, int(count), int(status))
        if not c["pinned"]:
            unpinned.setdefault(c["family"], []).append((c["index"], c["reason"], msg))
        elif msg is not None:
            wrong.append((c["index"], c["family"], msg))
    for fam, lst in unpinned.items():
        print("%s: unpinned in %s: %s" % (what, fam, lst))
        assert len(lst) <= UNPINNED_CAP * per_family[fam], (fam, lst)
    assert not wrong, wrong
    return sum(len(v) for v in unpinned.values())


# ------------------------------------------------------------------------------------------------ inputs of the GPU tests
def raw_batch(B, n_max, d, seed):
    """Ragged point sets with a keep mask with holes: an exact repeat of a point in every second set, lattice sets
    (integers in -2 .. 2: faces with many points, so the filter drops within a round and across rounds) for every third,
    one flat set per batch of more than one (set B // 2: last coordinate constant; in d = 1 a single repeated point)."""
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((B, n_max, d)) * rng.choice([1.0, 1e-2, 1e3], size=(B, 1, 1)) + 3.0 * rng.standard_normal((B, 1, d))
    n = rng.integers(min(n_max, d + 1), n_max + 1, size=B).astype(np.int32)
    n[0] = n_max
    for p in range(B):
        if p % 3 == 2:
            X[p] = rng.integers(-2, 3, (n_max, d)).astype(float)
        if p % 2 and n[p] > 3:
            X[p, 3] = X[p, 0]
    if B > 1:
        X[B // 2, :, -1] = 0.25
    keep = np.zeros(B, np.uint64)
    for p in range(B):
        mask = rng.random(64) < 0.85
        mask[:min(d + 1, 64)] = True
        keep[p] = keep_word(mask)
    keep[0] = np.uint64(2 ** 64 - 1)
    for p in range(B):
        X[p, n[p]:] = 0.0
    return X, n, keep
