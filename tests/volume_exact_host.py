"""Host build of polytope_amd/csrc/plp_volume_exact.hpp (tests/cabi/volume_exact_host.cpp, g++ -ffp-contract=off) and what
tests/test_volume_exact_host.py (CPU: the sequential rule against closed forms, its own identities and the reference) and
tests/test_volume_exact_gpu.py (the kernel against the host build bit for bit, the public volume_exact_batch against the
fixture) share: the named polytopes with their exact volumes, the fixture tests/golden/g30_volume_exact.npz, the
comparison rule and the cap on cases left out of it."""
import ctypes as C
import itertools
import math
import os

import numpy as np

import host_build as hb
from host_build import ROOT, ptr as _p

SRC = os.path.join(ROOT, "tests", "cabi", "volume_exact_host.cpp")

VS_OK, VS_UNBOUNDED, VS_EMPTY, VS_FLAT = 0, 1, 2, 3
# the comparison with the fixture: within SIGMAS sampling deviations of the reference's volume(); where the reference's
# extreme() had an answer, HULL_REL relative plus HULL_ABS * scale^d of scipy's hull volume of its vertices (a facet moved by
# eps = 1e-7, what reduce() may do, moves the volume by eps + 1e-15 / eps <= 1e-8 relative)
SIGMAS, HULL_REL, HULL_ABS = 5.0, 1e-8, 1e-12
# cases that miss the hull comparison are listed with their cause: at most this share of the flat family, none of any other
MISS_CAP = {"flat": 0.10}


def build(tmpdir, as_path=False):
    """Compiles the host build into tmpdir -> the loaded library, or (as_path) the path of the shared object."""
    out = hb.build(SRC, "libvolume_exact_host.so", tmpdir)
    return out if as_path else load(out)


def build_program(tmpdir):
    """The stand-alone program (-DVOLUME_EXACT_HOST_MAIN) under -fsanitize=address,undefined -> its path."""
    return hb.build_program(SRC, "VOLUME_EXACT_HOST_MAIN", "volume_exact_host_san", tmpdir)


def load(out):
    L = C.CDLL(out)
    L.volume_exact_host.restype = C.c_int
    L.volume_exact_host.argtypes = [C.c_longlong, C.c_int, C.c_int] + [C.c_void_p] * 9
    return L


def prep(A, b, m=None, keep=None, xc=None, scale=None):
    """The arguments as the contiguous arrays both builds take."""
    A = np.ascontiguousarray(A, dtype=np.float64)
    B, m_max, d = A.shape
    b = np.ascontiguousarray(b, dtype=np.float64).reshape(B, m_max)
    m = None if m is None else np.ascontiguousarray(m, dtype=np.int32).reshape(B)
    keep = None if keep is None else np.ascontiguousarray(keep, dtype=np.uint64).reshape(B)
    xc = None if xc is None else np.ascontiguousarray(xc, dtype=np.float64).reshape(B, d)
    scale = None if scale is None else np.ascontiguousarray(scale, dtype=np.float64).reshape(B)
    return A, b, m, keep, xc, scale


def run(L, A, b, m=None, keep=None, xc=None, scale=None, areas=True):
    """plp_vol_exact_batch on the host -> (volume[B], area[B, m_max] or None, status[B])."""
    A, b, m, keep, xc, scale = prep(A, b, m, keep, xc, scale)
    B, m_max, d = A.shape
    vol, status = np.empty(B), np.empty(B, np.int32)
    area = np.empty((B, m_max)) if areas else None
    rc = L.volume_exact_host(B, m_max, d, _p(A), _p(b), _p(m), _p(keep), _p(xc), _p(scale), _p(vol), _p(area), _p(status))
    assert rc == 0
    return vol, area, status


def one(L, A, b, **kw):
    """One polytope -> (volume, area[m], status)."""
    A = np.asarray(A, float)
    kw = {k: (None if v is None else np.asarray(v)[None]) for k, v in kw.items()}
    vol, area, status = run(L, A[None], np.asarray(b, float)[None], **kw)
    return float(vol[0]), area[0], int(status[0])


# ------------------------------------------------------------------------------------------------ closed forms
def cube(d, half=1.0):
    return np.vstack([np.eye(d), -np.eye(d)]), np.full(2 * d, half)


def cross(d):
    S = np.array(list(itertools.product([-1.0, 1.0], repeat=d)))
    return S, np.ones(len(S))


def simplex(d):
    return np.vstack([-np.eye(d), np.ones((1, d))]), np.r_[np.zeros(d), 1.0]


def cell24():
    """The 24-cell {|x_i| + |x_j| <= 1, i < j}: vertices the permutations of (+-1, 0, 0, 0) and (+-1/2)^4, volume 2."""
    rows = []
    for i, j in itertools.combinations(range(4), 2):
        for si, sj in itertools.product([-1.0, 1.0], repeat=2):
            r = np.zeros(4)
            r[i], r[j] = si, sj
            rows.append(r)
    return np.array(rows), np.ones(24)


def cube_pyramid():
    """The pyramid in R^4 over the cube [-1, 1]^3 x {0} with apex (0, 0, 0, 1): volume 8 / 4 = 2."""
    rows, rhs = [np.r_[0.0, 0, 0, -1]], [0.0]
    for k in range(3):
        for s in (-1.0, 1.0):
            r = np.zeros(4)
            r[k], r[3] = s, 1.0
            rows.append(r)
            rhs.append(1.0)
    return np.array(rows), np.array(rhs)


def closed_forms():
    """[(name, A, b, exact volume)] in d = 1 .. 4."""
    out = [("interval", np.array([[2.0], [-1.0]]), np.array([3.0, 0.25]), 1.75)]
    for d in (2, 3, 4):
        A, b = cube(d, 0.75)
        out.append(("cube %d" % d, A, b, 1.5 ** d))
        A, b = cross(d)
        out.append(("cross %d" % d, A, b, 2.0 ** d / math.factorial(d)))
        A, b = simplex(d)
        out.append(("simplex %d" % d, A, b, 1.0 / math.factorial(d)))
    A, b = cell24()
    out.append(("24-cell", A, b, 2.0))
    A, b = cube_pyramid()
    out.append(("pyramid over a cube", A, b, 2.0))
    out.append(("square pyramid", np.array([[0, 0, -1], [1, 0, 1], [-1, 0, 1], [0, 1, 1], [0, -1, 1]], float),
                np.array([0, 1, 1, 1, 1.0]), 4.0 / 3.0))
    return out


# ------------------------------------------------------------------------------------------------ the fixture
def fixture():
    """tests/golden/g30_volume_exact.npz (tests/golden/make_golden_volume_exact.py) -> a list of dicts: family, shape index,
    d, A, b (the reference's constructor-normalised rows), unbounded / flat (by the reference: a side of its bounding box is
    infinite; its Chebyshev radius is <= 1e-7), vol_mc (its volume(P, nsamples=N, seed)), box (the volume of the bounding
    box it sampled), N, vol_hull (scipy's hull volume of its extreme(), NaN where it had no answer in three calls)."""
    z = np.load(os.path.join(ROOT, "tests", "golden", "g30_volume_exact.npz"), allow_pickle=False)
    z = {k: z[k] for k in z.files}
    fams = [str(s) for s in z["families"]]
    out = []
    for c in range(len(z["family"])):
        d = int(z["d"][c])
        lo, hi = z["row_off"][c], z["row_off"][c + 1]
        out.append(dict(index=c, family=fams[z["family"][c]], d=d, A=z["A"][z["a_off"][c]:z["a_off"][c + 1]].reshape(hi - lo, d),
                        b=z["b"][lo:hi], unbounded=bool(z["unbounded"][c]), flat=bool(z["flat"][c]),
                        vol_mc=float(z["vol_mc"][c]), box=float(z["box"][c]), N=int(z["N"][c]), vol_hull=float(z["vol_hull"][c]),
                        extent=float(z["extent"][c])))
    return out


def pack(cases, d, m_max=None):
    """The cases of dimension d as one packed batch -> (indices into `cases`, A[B, m_max, d], b[B, m_max], m[B]); padding
    rows are zero."""
    sel = [i for i, c in enumerate(cases) if c["d"] == d]
    m = np.array([cases[i]["A"].shape[0] for i in sel], np.int32)
    m_max = int(m.max()) if m_max is None else m_max
    A = np.zeros((len(sel), m_max, d))
    b = np.zeros((len(sel), m_max))
    for k, i in enumerate(sel):
        A[k, :m[k]] = cases[i]["A"]
        b[k, :m[k]] = cases[i]["b"]
    return sel, A, b, m


def sigma(case):
    """The standard deviation of the reference's estimate, from the estimate itself: box sqrt(p (1 - p) / N) with
    p = vol_mc / box (p (1 - p) not below 1 / N: one sample)."""
    p = min(max(case["vol_mc"] / case["box"], 0.0), 1.0)
    return case["box"] * math.sqrt(max(p * (1.0 - p), 1.0 / case["N"]) / case["N"])


def check_cases(cases, results, what):
    """results[i] = (volume, status) of case i, as the public call gives them.  Every bounded, full-dimensional case within
    SIGMAS sigma of the reference's estimate; with the hull volume where there is one, misses listed and capped."""
    wrong, missed, per_family = [], {}, {}
    worst_sigma = worst_hull = 0.0
    for c, (vol, status) in zip(cases, results):
        fam = c["family"]
        per_family[fam] = per_family.get(fam, 0) + 1
        if c["flat"] or c["unbounded"]:
            want = VS_FLAT if c["flat"] else VS_UNBOUNDED
            if status != want:
                wrong.append((c["index"], fam, "status %d for %d" % (status, want)))
            continue
        if status != VS_OK or not np.isfinite(vol):
            wrong.append((c["index"], fam, "status %d, volume %r" % (status, vol)))
            continue
        z = abs(vol - c["vol_mc"]) / sigma(c)
        worst_sigma = max(worst_sigma, z)
        if z > SIGMAS:
            wrong.append((c["index"], fam, "%.2f sigma from the sampled volume (%r, %r)" % (z, vol, c["vol_mc"])))
        if np.isfinite(c["vol_hull"]):
            err = abs(vol - c["vol_hull"])
            tol = HULL_REL * abs(c["vol_hull"]) + HULL_ABS * c["extent"] ** c["d"]
            worst_hull = max(worst_hull, err / tol)
            if err > tol:
                missed.setdefault(fam, []).append((c["index"], "hull %r, ours %r: %.1e of the bound" % (c["vol_hull"], vol, err / tol)))
    print("%s: worst %.2f sigma, worst hull error %.2e of its bound" % (what, worst_sigma, worst_hull))
    for fam, lst in missed.items():
        print("%s: misses the hull volume in %s: %s" % (what, fam, lst))
        assert len(lst) <= MISS_CAP.get(fam, 0.0) * per_family[fam], (fam, lst)
    assert not wrong, wrong
    return worst_sigma, worst_hull
