"""Host build of polytope_amd/csrc/plp_extreme.hpp (tests/cabi/extreme_host.cpp, g++ -ffp-contract=off) and what
tests/test_extreme_host.py (CPU: the sequential rule against the reference's extreme()) and tests/test_extreme_gpu.py (the
kernel against the host build bit for bit, the public extreme_batch against the fixture) share: the fixture
tests/golden/g29_extreme.npz, the comparison rule and the cap on cases left out of it."""
import ctypes as C
import os

import numpy as np

import host_build as hb
from host_build import ROOT, keep_word, ptr as _p, upper_bound as vmax_for  # noqa: F401

SRC = os.path.join(ROOT, "tests", "cabi", "extreme_host.cpp")

XS_OK, XS_OVERFLOW, XS_EMPTY, XS_FLAT, XS_UNBOUNDED = 0, 1, 2, 3, 4
ABS_TOL = 1e-7
# what the reference's extreme() did with a case (the fixture's `ref_kind`)
REF_ROWS, REF_NONE, REF_RAISED = 0, 1, 2
# the comparison with the fixture, as sets: the reference's rows collapsed at COLLAPSE of the extent E = max(1, |V|_inf)
# (its repeats of a degenerate vertex agree to rounding), then equal counts and every vertex within MATCH E of one of the
# other side's
COLLAPSE, MATCH = 1e-7, 1e-8
# cases left out of the comparison (`pinned` false in the fixture, with a reason code): at most this share of the flat
# family and none of any other
UNPINNED_CAP = {"flat": 0.10}


def build(tmpdir, as_path=False):
    """Compiles the host build into tmpdir -> the loaded library, or (as_path) the path of the shared object."""
    out = hb.build(SRC, "libextreme_host.so", tmpdir)
    return out if as_path else load(out)


def build_program(tmpdir):
    """The stand-alone program (-DEXTREME_HOST_MAIN) under -fsanitize=address,undefined -> its path."""
    return hb.build_program(SRC, "EXTREME_HOST_MAIN", "extreme_host_san", tmpdir)


def load(out):
    L = C.CDLL(out)
    L.extreme_host.restype = C.c_int
    L.extreme_host.argtypes = [C.c_longlong, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                               C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.extreme_unrank_mismatches.restype = C.c_longlong
    L.extreme_unrank_mismatches.argtypes = [C.c_int]
    return L


def run(L, A, b, m=None, keep=None, v_max=None, basis=True):
    """plp_extreme_batch on the host -> (V[B, v_max, d], count[B], basis[B, v_max, d] or None, status[B])."""
    A = np.ascontiguousarray(A, dtype=np.float64)
    B, m_max, d = A.shape
    b = np.ascontiguousarray(b, dtype=np.float64).reshape(B, m_max)
    m = None if m is None else np.ascontiguousarray(m, dtype=np.int32)
    keep = None if keep is None else np.ascontiguousarray(keep, dtype=np.uint64)
    v_max = vmax_for(d, m_max) if v_max is None else v_max
    V = np.empty((B, v_max, d))
    count, status = np.empty(B, np.int32), np.empty(B, np.int32)
    bas = np.empty((B, v_max, d), np.int32) if basis else None
    rc = L.extreme_host(B, m_max, d, _p(A), _p(b), _p(m), _p(keep), v_max, _p(V), _p(count), _p(bas), _p(status))
    assert rc == 0
    return V, count, bas, status


# ------------------------------------------------------------------------------------------------ the fixture
def fixture():
    """tests/golden/g29_extreme.npz (tests/golden/make_golden_extreme.py) -> a list of dicts: family, shape (the soak
    shape, or the row count and dimension of a named case), A, b (the reference's constructor-normalised rows), ref_kind
    (REF_*) and R (the rows extreme() returned) of the first of `calls` calls that had an answer, or of the first call when
    none had (R may then hold inf / nan), no_answer (the calls in which it returned None, raised or wrote inf / nan),
    pinned, reason."""
    z = np.load(os.path.join(ROOT, "tests", "golden", "g29_extreme.npz"), allow_pickle=False)
    z = {k: z[k] for k in z.files}
    fams = [str(s) for s in z["families"]]
    out = []
    for c in range(len(z["family"])):
        d = int(z["d"][c])
        lo, hi = z["row_off"][c], z["row_off"][c + 1]
        vlo, vhi = z["ref_off"][c], z["ref_off"][c + 1]
        out.append(dict(index=c, family=fams[z["family"][c]], d=d,
                        A=z["A"][z["a_off"][c]:z["a_off"][c + 1]].reshape(hi - lo, d), b=z["b"][lo:hi],
                        ref_kind=int(z["ref_kind"][c]), R=z["R"][z["r_off"][c]:z["r_off"][c + 1]].reshape(vhi - vlo, d),
                        pinned=bool(z["pinned"][c]), reason=int(z["reason"][c]), no_answer=int(z["no_answer"][c]),
                        calls=int(z["calls"])))
    return out


def pack(cases, d):
    """The cases of dimension d as one packed batch -> (indices into `cases`, A[B, m_max, d], b[B, m_max], m[B]); padding
    rows are zero."""
    sel = [i for i, c in enumerate(cases) if c["d"] == d]
    m = np.array([cases[i]["A"].shape[0] for i in sel], np.int32)
    A = np.zeros((len(sel), int(m.max()), d))
    b = np.zeros((len(sel), int(m.max())))
    for k, i in enumerate(sel):
        A[k, :m[k]] = cases[i]["A"]
        b[k, :m[k]] = cases[i]["b"]
    return sel, A, b, m


def collapse(R):
    """The reference's rows with its repeats of one vertex taken out (greedy, COLLAPSE of the extent) -> (rows, extent)."""
    E = max(1.0, float(np.abs(R).max())) if R.size else 1.0
    out = []
    for q in R:
        if not any(np.max(np.abs(q - w)) <= COLLAPSE * E for w in out):
            out.append(q)
    return np.array(out).reshape(-1, R.shape[1]), E


def compare(case, V, count, status):
    """One case against the fixture -> None, or what is wrong (a string).  V[count, d]: our vertices."""
    R, kind = case["R"], case["ref_kind"]
    # extreme() is not repeatable where it has no answer, so the fixture holds several calls: FLAT / UNBOUNDED is right only
    # where one of them returned None, raised or wrote inf / nan; vertices only where one of them returned finite rows (R)
    lost, calls = case["no_answer"], case["calls"]
    if status in (XS_FLAT, XS_UNBOUNDED):
        return None if lost > 0 else "status %d where the reference has %d rows" % (status, len(R))
    if lost == calls:
        return "status %d, %d vertices where the reference has no answer (kind %d)" % (status, count, kind)
    assert kind == REF_ROWS and np.all(np.isfinite(R))
    if status != XS_OK:
        return "status %d" % status
    Rd, E = collapse(R)
    ours = V[:count]
    if len(Rd) != count:
        return "%d vertices for the reference's %d (%d rows)" % (count, len(Rd), len(R))
    e1 = max(np.min(np.max(np.abs(ours - q), axis=1)) for q in Rd) / E
    e2 = max(np.min(np.max(np.abs(Rd - v), axis=1)) for v in ours) / E
    if e1 > MATCH or e2 > MATCH:
        return "vertices off by %.1e / %.1e of the extent" % (e1, e2)
    return None


def check_cases(cases, results, what):
    """results[i] = (V, count, status) of case i.  Pinned cases must compare clean; unpinned ones are listed with their
    reason, and their number is held to UNPINNED_CAP.  -> the number of unpinned cases."""
    wrong, unpinned = [], {}
    per_family = {}
    for c, (V, count, status) in zip(cases, results):
        per_family[c["family"]] = per_family.get(c["family"], 0) + 1
        msg = compare(c, V, int(count), int(status))
        if not c["pinned"]:
            unpinned.setdefault(c["family"], []).append((c["index"], c["reason"], msg))
        elif msg is not None:
            wrong.append((c["index"], c["family"], msg))
    for fam, lst in unpinned.items():
        print("%s: unpinned in %s: %s" % (what, fam, lst))
        assert len(lst) <= UNPINNED_CAP.get(fam, 0.0) * per_family[fam], (fam, lst)
    assert not wrong, wrong
    return sum(len(v) for v in unpinned.values())
