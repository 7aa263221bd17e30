"""Host build of polytope_amd/csrc/plp_support.hpp (tests/cabi/support_host.cpp, g++ -ffp-contract=off) and the inputs
tests/test_support_host.py (CPU: the per-LP function against the oracle's simplex) and tests/test_support_gpu.py (device
answers against the host build bit for bit, and against the oracle) share: families, seeds, directions, oracle answers."""
import ctypes as C
import functools
import os

import numpy as np

import host_build as hb

ROOT = hb.ROOT
SRC = os.path.join(ROOT, "tests", "cabi", "support_host.cpp")

# (m_max, d) of the random families; the seed of family k is SEED0 + k (kept here: the GPU tests reuse them)
SHAPES = ((5, 1), (7, 2), (16, 3), (17, 3), (33, 4), (64, 4))
SEED0 = 4100
B_FAMILY = 40
K_RANDOM = 9
HANDBACK_CAP = 0.01   # raw status 1 on the random bounded family, as a share of its LPs

# The soak families (scripts/soak_lane.py: make) and the shapes they are run at: walk3 at d = 1, 2, 3 and walk4 at d = 4, each
# of the 16 / 32 / 64 row-slot instances twice, (32, 4) and (48, 4) being where status-0 answers were found wrong.
FAMILIES = ("random", "ragged", "unbounded", "dup", "scaled", "flat", "lattice")
SOAK_SHAPES = ((16, 1), (17, 2), (16, 3), (64, 3), (32, 4), (48, 4))
# the run that found them: these shapes, 7 random directions + -e_i after each shape's polytopes, one generator throughout;
# `dup` at seed 7: (48, 4) polytope 29 directions 5 and 8, (32, 4) polytope 6 direction 3; seed 8: (48, 4) polytope 17 direction 5
FOUND_SHAPES = ((16, 3), (12, 2), (32, 4), (24, 3), (48, 4), (8, 1))
FOUND = ((7, (48, 4), 29, 5), (7, (48, 4), 29, 8), (7, (32, 4), 6, 3), (8, (48, 4), 17, 5))
B_SOAK = 30
K_SOAK = 7
# (the seeds tests/test_verify_host.py runs the families at; `dup` at 7 is one of the streams with wrong status-0 answers)
FAMILY_SEED = {"random": 1, "ragged": 2, "unbounded": 3, "scaled": 4, "flat": 5, "lattice": 6, "dup": 7}
# raw status 1 as a share of the LPs of polytopes that have a centre: the families of well-separated rows, and the ones with
# rows a hair apart, slabs of no width and degenerate vertices (where a walk that is not sure hands back)
HANDBACK_CAPS = {"random": 0.01, "ragged": 0.01, "unbounded": 0.01, "scaled": 0.01, "lattice": 0.01,
                 "dup": 0.10, "flat": 0.10, "degenerate": 0.10}


def build(tmpdir, as_path=False):
    """Compiles the host build into tmpdir -> the loaded library, or (as_path) the path of the shared object."""
    out = hb.build(SRC, "libsupport_host.so", tmpdir)
    return out if as_path else load(out)


def build_program(tmpdir):
    return hb.build_program(SRC, "SUPPORT_HOST_MAIN", "support_host_asan", tmpdir)


def load(out):
    L = C.CDLL(out)
    L.support_host.restype = C.c_int
    L.support_host.argtypes = [C.c_longlong, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p,
                               C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.support_polytopes_per_group.restype = C.c_int
    L.support_polytopes_per_group.argtypes = [C.c_int, C.c_int]
    return L


def run(L, A, b, C_, xc, m=None, points=True):
    """plp_support_batch on the host -> (h[B, K], x[B, K, d] or None, status[B, K]), raw statuses."""
    A = np.ascontiguousarray(A, dtype=np.float64)
    B, m_max, d = A.shape
    b = np.ascontiguousarray(b, dtype=np.float64).reshape(B, m_max)
    C_ = np.ascontiguousarray(C_, dtype=np.float64)
    K = C_.shape[-2]
    xc = np.ascontiguousarray(xc, dtype=np.float64).reshape(B, d)
    m = None if m is None else np.ascontiguousarray(m, dtype=np.int32)
    h = np.empty((B, K))
    x = np.empty((B, K, d)) if points else None
    st = np.empty((B, K), np.int32)
    rc = L.support_host(B, m_max, d, hb.ptr(A), hb.ptr(b), hb.ptr(m), K, hb.ptr(C_), 1 if C_.ndim == 2 else 0, hb.ptr(xc), hb.ptr(h),
                        hb.ptr(x), hb.ptr(st))
    assert rc == 0
    return h, x, st


def _soak_lane():
    import sys
    scripts = os.path.join(ROOT, "scripts")
    if scripts not in sys.path:
        sys.path.insert(0, scripts)
    import soak_lane
    return soak_lane


def family(k, B=B_FAMILY, bounded=True, ragged=True, rng=None, shape=None):
    """Family k of SHAPES: random_hpolytopes with ragged row counts (rows beyond m[p] zeroed) -> A, b, m.
    k a name of FAMILIES: soak_lane.make(rng, B, *shape, k), the generator every other kernel family is soaked on (rows
    beyond m[p] are left as made: nothing may read them)."""
    if isinstance(k, str):
        return _soak_lane().make(rng, B, shape[0], shape[1], k)
    from polytope_amd.synth import random_hpolytopes
    m_max, d = SHAPES[k]
    A, b = random_hpolytopes(B, m_max, d, seed=SEED0 + k, bounded=bounded)
    m = np.full(B, m_max, np.int32)
    if ragged:
        lo = min(m_max, 2 * d if bounded else 1)
        m = np.random.default_rng(SEED0 + 100 + k).integers(lo, m_max + 1, size=B).astype(np.int32)
        m[0] = m_max
        for p in range(B):
            A[p, m[p]:] = 0.0
            b[p, m[p]:] = 0.0
    return A, b, m


def directions(k, B, shared, K=K_RANDOM, axes=True):
    """K random directions plus +-e_i: [K + 2 d, d] shared, or [B, K + 2 d, d]."""
    d = SHAPES[k][1]
    rng = np.random.default_rng(SEED0 + 200 + k + (50 if shared else 0))
    R = rng.standard_normal((K, d) if shared else (B, K, d))
    if not axes:
        return R
    E = np.vstack([np.eye(d), -np.eye(d)])
    return np.vstack([R, E]) if shared else np.concatenate([R, np.broadcast_to(E, (B, 2 * d, d))], axis=1)


def tie_directions(A, m, seed):
    """Directions chosen to tie, per polytope [B, 7, d]: with (i, j) the two live rows closest in angle (on `dup` a pair a
    hair apart) and k a random live row, k2 the row nearest to it:  a_i, a_j, a_k (a whole facet is optimal),  a_i + a_j,
    a_k + a_k2 (a ridge),  -a_i, -a_k.  A polytope of one row repeats it; one of none gets zeros."""
    B, _, d = A.shape
    rng = np.random.default_rng(seed)
    T = np.zeros((B, 7, d))
    for p in range(B):
        mp = int(m[p])
        k = int(rng.integers(0, max(mp, 1)))
        if mp < 1:
            continue
        R = A[p, :mp]
        nrm = np.linalg.norm(R, axis=1)
        U = R / np.where(nrm > 0, nrm, 1.0)[:, None]
        G = U @ U.T - 2.0 * np.eye(mp)
        i, j = np.unravel_index(int(np.argmax(G)), G.shape) if mp > 1 else (0, 0)
        k2 = int(np.argmax(G[k]))
        T[p] = [R[i], R[j], R[k], R[i] + R[j], R[k] + R[k2], -R[i], -R[k]]
    return T


def centres(O, A, b, m, strict=True):
    """Chebyshev centres by the oracle.  strict: every polytope has one (the random families).  Otherwise a polytope whose
    ball LP does not end with r > 0 (empty, flat, an unbounded ball) keeps a centre of NaNs: the kernel hands all of it back."""
    xc = np.zeros((A.shape[0], A.shape[2]))
    for p in range(A.shape[0]):
        st, r, c = O.cheby(A[p, :m[p]], b[p, :m[p]])
        if strict:
            assert st == 0 and r > 0
        xc[p] = c if st == 0 and r > 0 else np.nan
    return xc


def soak_cases(O, fam, seed, shapes=SOAK_SHAPES, B=B_SOAK, K=K_SOAK, translate=0.0):
    """One generator default_rng(seed) carried through `shapes`: per shape the polytopes of soak family `fam`, then K
    standard-normal directions, + -e_i appended (C shared, [K + 2 d, d]); the tie directions and two more random ones per
    polytope (C per polytope, [B, 9, d]) come from generators of their own, so the stream is the one of FOUND_SHAPES.
    translate: b += A t with |t| = translate, t random per polytope -- beta = b - a.xc then cancels at that extent.
    -> a list of dicts: shape, A, b, m, xc (NaN rows: no centre), and per layout C, the oracle's status, h and |x|_max."""
    rng = np.random.default_rng(seed)
    out = []
    for s, (m_max, d) in enumerate(shapes):
        A, b, m = family(fam, B=B, rng=rng, shape=(m_max, d))
        Cs = np.vstack([rng.standard_normal((K, d)), np.eye(d), -np.eye(d)])
        own = np.random.default_rng([seed, s, 77])
        if translate:
            t = own.standard_normal((B, d))
            t *= translate / np.linalg.norm(t, axis=1, keepdims=True)
            b = b + np.einsum("pik,pk->pi", A, t)
        Co = np.concatenate([tie_directions(A, m, [seed, s, 78]), own.standard_normal((B, 2, d))], axis=1)
        out.append(_case(O, A, b, m, Cs, Co))
    return out


def _case(O, A, b, m, Cs, Co):
    case = {"shape": A.shape[1:], "A": A, "b": b, "m": m, "xc": centres(O, A, b, m, strict=False)}
    for name, C_ in (("shared", Cs), ("own", Co)):
        ost, oh, ox = oracle_support(O, A, b, m, C_, extent=True)
        case[name] = (C_, ost, oh, ox)
    return case


def degenerate_cases(O):
    """Degenerate vertices at d <= 4, in the format of soak_cases: the pyramids of tests/test_gpu_parity.py (many facets
    through one apex, some nearly parallel), the structured (16, 3) polytopes of tests/structured_cases.py (cubes with
    duplicated, tangent and near-tolerance rows, vertex fans, ulp twins) and the polytopes of tests/degenerate_cases.py
    (a vertex fan, cubes with every row twice as ball LPs in d + 1 columns, a single point, a barely empty set).
    Directions: 9 random ones + -e_i shared; per polytope the tie directions, two random ones and, where the case is
    an LP, its own cost."""
    from degenerate_cases import degenerate_lps
    from structured_cases import structured_polytopes
    from test_gpu_parity import _pyramids
    rng = np.random.default_rng(4242)
    batches = []
    for (m_max, d) in ((14, 2), (16, 3), (24, 4)):
        A, b = _pyramids(B_SOAK, m_max, d, rng)
        batches.append((A, b, np.zeros((B_SOAK, 1, d))))
    A, b, _ = structured_polytopes(32)
    batches.append((A, b, np.zeros((32, 1, 3))))
    by_shape = {}
    for _, c, G, h in degenerate_lps(dims=(2, 3, 4), reps=6):
        if G.shape[1] <= 4:
            by_shape.setdefault(G.shape, []).append((G, h, -c))
    for lps in by_shape.values():
        batches.append((np.stack([g for g, _, _ in lps]), np.stack([h for _, h, _ in lps]), np.stack([c for _, _, c in lps])[:, None, :]))
    out = []
    for s, (A, b, cost) in enumerate(batches):
        B, m_max, d = A.shape
        m = np.full(B, m_max, np.int32)
        Cs = np.vstack([rng.standard_normal((9, d)), np.eye(d), -np.eye(d)])
        Co = np.concatenate([tie_directions(A, m, [4242, s]), rng.standard_normal((B, 2, d)), cost], axis=1)
        out.append(_case(O, np.ascontiguousarray(A), np.ascontiguousarray(b), m, Cs, Co))
    return out


def run_case(L, case, layout, points=True):
    """The host build on one layout of a case -> h, x, st."""
    return run(L, case["A"], case["b"], case[layout][0], case["xc"], case["m"], points=points)


def oracle_off_fixture():
    """tests/golden/found/support/oracle_off.npz (tests/golden/make_support_found.py) -> [(name, A, b, c, xc, h_exact, extent)]:
    the soak's LPs on which the oracle is beyond tolerance of the exact rational optimum."""
    z = np.load(os.path.join(ROOT, "tests", "golden", "found", "support", "oracle_off.npz"))
    out = [None] * len(z["names"])
    for key in z.files:
        if key.startswith("idx_"):
            tag = key[4:]
            for q, i in enumerate(z[key]):
                out[i] = (str(z["names"][i]), z["A_" + tag][q], z["b_" + tag][q], z["c_" + tag][q], z["xc_" + tag][q],
                          float(z["h_exact"][i]), float(z["extent"][i]))
    return out


def check_case(case, layout, h, x, st, counts=None):
    """What every answer the kernel does not hand back must satisfy (check_against_oracle with the extent rule), and what
    the statuses may be: a polytope without a centre comes back as 1 in every direction; 3 only where the oracle says 3, and
    never 0 there.  counts: [LPs of polytopes that have a centre, handed back among them] is added to."""
    C_, ost, oh, ox = case[layout]
    has = np.isfinite(case["xc"]).all(axis=1)
    assert np.all(st[~has] == 1)
    assert set(np.unique(st)) <= {0, 1, 3}
    assert np.all(np.isnan(h[st == 1])) and (x is None or np.all(np.isnan(x[st == 1])))
    assert np.all(h[st == 3] == np.inf)
    assert not np.any((ost == 3) & (st == 0)) and not np.any((ost == 0) & (st == 3))
    check_against_oracle(case["A"], case["b"], case["m"], C_, h, x, st, ost, oh, where=(st != 1), ext=ox)
    if counts is not None:
        counts[0] += int(has.sum()) * st.shape[1]
        counts[1] += int((st[has] == 1).sum())


def oracle_support(O, A, b, m, C_, extent=False):
    """(status[B, K], h[B, K]) by the oracle's simplex: min -c.x; h = -fun where the status is 0, NaN elsewhere.
    extent: also |x|_max of the oracle's optimal point (NaN elsewhere)."""
    B = A.shape[0]
    K = C_.shape[-2]
    st = np.zeros((B, K), np.int32)
    h = np.full((B, K), np.nan)
    xm = np.full((B, K), np.nan)
    for p in range(B):
        mp = A.shape[1] if m is None else int(m[p])
        for j in range(K):
            c = C_[j] if C_.ndim == 2 else C_[p, j]
            s, xo, fun, _ = O.lp_solve(-c, A[p, :mp], b[p, :mp])
            st[p, j] = s
            if s == 0:
                h[p, j] = -fun
                xm[p, j] = np.max(np.abs(xo))
    return (st, h, xm) if extent else (st, h)


def exact_support(A, b, c, xc):
    """h_P(c) = max { c.x : A x <= b } in EXACT rational arithmetic on the doubles as stored (no entry is dropped, nothing is
    rounded): the arbiter where the kernel and the oracle differ on rows a hair apart -- the oracle, like HiGHS, reads matrix
    entries <= 1e-9 as zero and accepts points 1e-9 outside a row.  xc: a strictly interior point (the start).  Dictionary
    simplex with Bland's rule, the d free variables x' = x - xc enter once and never leave: m rows x (d + 1) columns.
    -> (h as a Fraction, x as Fractions), or (None, None) where P is unbounded in the direction c."""
    from fractions import Fraction as F
    A = [[F(float(v)) for v in row] for row in np.asarray(A)]
    m, d = len(A), len(c)
    xc = [F(float(v)) for v in xc]
    cc = [F(float(v)) for v in c]
    beta = [F(float(b[i])) - sum(A[i][k] * xc[k] for k in range(d)) for i in range(m)]
    assert all(v > 0 for v in beta), "the start is not strictly inside"
    # basic variable of row i = const[i] + sum_j T[i][j] * nonbasic[j];  variables: 0 .. d - 1 free, d + i the slack of row i
    T = [[-A[i][k] for k in range(d)] for i in range(m)]
    const = list(beta)
    basic, nonbasic = [d + i for i in range(m)], list(range(d))
    g, z0 = list(cc), F(0)
    for _ in range(100000):
        cand = [(nonbasic[j], j) for j in range(d) if (g[j] != 0 if nonbasic[j] < d else g[j] > 0)]
        if not cand:
            break
        _, j = min(cand)
        sgn = 1 if g[j] > 0 else -1
        best = None
        for i in range(m):
            if basic[i] >= d and T[i][j] * sgn < 0:
                ratio = const[i] / (-T[i][j] * sgn)
                if best is None or (ratio, basic[i]) < best[:2]:
                    best = (ratio, basic[i], i)
        if best is None:
            return None, None
        i = best[2]
        piv = T[i][j]
        # nonbasic[j] = (basic[i] - const[i] - sum_{k != j} T[i][k] N_k) / piv
        row = [-T[i][k] / piv for k in range(d)]
        row[j] = 1 / piv
        rc = -const[i] / piv
        for q in range(m):
            if q != i and T[q][j] != 0:
                f = T[q][j]
                const[q] += f * rc
                T[q] = [T[q][k] + f * row[k] if k != j else f * row[j] for k in range(d)]
        f = g[j]
        z0 += f * rc
        g = [g[k] + f * row[k] if k != j else f * row[j] for k in range(d)]
        T[i], const[i] = row, rc
        basic[i], nonbasic[j] = nonbasic[j], basic[i]
    else:
        raise RuntimeError("exact_support: no end")
    xp = [F(0)] * d
    for i in range(m):
        if basic[i] < d:
            xp[basic[i]] = const[i]
    x = [xc[k] + xp[k] for k in range(d)]
    return z0 + sum(cc[k] * xc[k] for k in range(d)), x


def check_against_oracle(A, b, m, C_, h, x, st, ost, oh, where=None, ext=None):
    """The tolerance of the support tests: status equal to the oracle's; where it is 0, |h - h_oracle| <= 1e-9 max(1, |h|),
    A x <= b + 1e-9 and |c.x - h| <= 1e-12 max(1, |h|).  `where`: the LPs to look at (default: all).
    ext (|x_oracle|_max per LP): the first two relative to the EXTENT max(1, |h|, ext) -- tests/test_verify_host.py: _ext, the
    rule the careful engine is held to: a value of 1.5 at a vertex 1e3 away is known to 1e-16 x 1e3."""
    sel = np.ones(st.shape, bool) if where is None else where
    assert np.array_equal(st[sel], ost[sel]), [(tuple(q), st[tuple(q)], ost[tuple(q)]) for q in np.argwhere(sel & (st != ost))[:5]]
    ok = sel & (st == 0)
    scale = np.maximum(1.0, np.abs(h)) if ext is None else np.fmax(np.maximum(1.0, np.abs(h)), ext)
    off = np.where(ok, np.abs(h - oh) / scale, 0.0)
    assert np.all(off <= 1e-9), [(tuple(q), h[tuple(q)], oh[tuple(q)]) for q in np.argwhere(off > 1e-9)[:8]]
    if x is None:
        return
    B, K = st.shape
    Cb = np.broadcast_to(C_, (B,) + C_.shape) if C_.ndim == 2 else C_
    cx = np.einsum("pjk,pjk->pj", Cb, x)
    assert np.all(np.abs(cx[ok] - h[ok]) <= 1e-12 * np.maximum(1.0, np.abs(h[ok])))
    Ax = np.einsum("pik,pjk->pji", A, x)   # [B, K, m_max]
    rows = np.arange(A.shape[1])[None, None, :] < (np.full(B, A.shape[1]) if m is None else m)[:, None, None]
    viol = np.where(rows, Ax - b[:, None, :], -np.inf).max(axis=2)
    assert np.all(viol[ok] <= 1e-9 * (1.0 if ext is None else scale[ok])), viol[ok].max()


@functools.lru_cache(maxsize=None)
def _cached(key):
    return {}


def memo(key, make):
    """One value per key for the whole test session (oracle answers are computed once and shared)."""
    slot = _cached(key)
    if "v" not in slot:
        slot["v"] = make()
    return slot["v"]
