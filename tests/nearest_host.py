"""Host build of polytope_amd/csrc/plp_nearest.hpp (tests/cabi/nearest_host.cpp, g++ -ffp-contract=off) and what
tests/test_nearest_host.py (CPU: the per-problem function against references written out here) and tests/test_nearest_gpu.py
(device answers against the host build bit for bit, resolved answers against the references) share: the loader, the input
families, the points, two references and the checks.

References (neither is the product's fallback, polytope_amd.batch._nearest_resolve; they share no code with it):
  reference()        plain numpy: the nearest point is the projection of p onto the affine hull of SOME subset of at most d
                     rows; every subset of the rows that can be active (slack at p below the distance of a known feasible
                     point) is projected onto with the pseudo-inverse, the feasible candidates kept, the closest taken.
  exact_reference()  the same enumeration in fractions.Fraction on the doubles as stored (m <= 12): the arbiter for rows a
                     hair apart."""
import ctypes as C
import itertools
import math
import os
import struct
import subprocess

import numpy as np

import host_build as hb
import support_host as sh

ROOT = hb.ROOT
SRC = os.path.join(ROOT, "tests", "cabi", "nearest_host.cpp")
FAMILIES = sh.FAMILIES
SOAK_SHAPES = sh.SOAK_SHAPES
HANDBACK_CAPS = sh.HANDBACK_CAPS
B_SOAK, K_SOAK = sh.B_SOAK, sh.K_SOAK
B_CPU = 10          # polytopes per shape of the CPU test's soak cases (the reference enumerates row subsets: (48, 4) is slow)
SEPARATED = ("random", "ragged", "unbounded", "scaled", "lattice")   # families of well-separated rows
TOL = 1e-9           # the project's LP tolerance (support_host.check_against_oracle), relative to the extent E
HILDRETH_SWEEPS = 60
REF_FEAS = 1e-12     # a candidate of reference() is feasible when no row is violated by more than this times E


def build(tmpdir):
    return load(hb.build(SRC, "libnearest_host.so", tmpdir))


def build_program(tmpdir):
    return hb.build_program(SRC, "NEAREST_HOST_MAIN", "nearest_host_asan", tmpdir)


def load(out):
    L = C.CDLL(out)
    L.nearest_host.restype = C.c_int
    L.nearest_host.argtypes = [C.c_longlong, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int,
                               C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    for name in ("nearest_polytopes_per_group", "nearest_chunk_points", "nearest_iter_cap"):
        getattr(L, name).restype = C.c_int
        getattr(L, name).argtypes = [C.c_int, C.c_int]
    return L


def run(L, A, b, X, m=None, points=True, faces=True):
    """plp_nearest_batch on the host, raw statuses -> dict(dist[B, K], x[B, K, d], face[B, K], lam[B, K, d], status[B, K])."""
    A = np.ascontiguousarray(A, dtype=np.float64)
    B, m_max, d = A.shape
    b = np.ascontiguousarray(b, dtype=np.float64).reshape(B, m_max)
    X = np.ascontiguousarray(X, dtype=np.float64)
    K = X.shape[-2]
    m = None if m is None else np.ascontiguousarray(m, dtype=np.int32)
    dist, st = np.empty((B, K)), np.empty((B, K), np.int32)
    x = np.empty((B, K, d)) if points else None
    face = np.empty((B, K), np.uint64) if faces else None
    lam = np.empty((B, K, d)) if faces else None
    rc = L.nearest_host(B, m_max, d, hb.ptr(A), hb.ptr(b), hb.ptr(m), K, hb.ptr(X), 1 if X.ndim == 2 else 0, hb.ptr(dist),
                        hb.ptr(x), hb.ptr(face), hb.ptr(lam), hb.ptr(st))
    assert rc == 0
    return dict(dist=dist, x=x, face=face, lam=lam, status=st)


def write_records(path, records):
    """The input of the stand-alone program: per record int64 B, m_max, d, K, x_shared, then A, b, m (int32), X."""
    with open(path, "wb") as f:
        for A, b, m, X in records:
            B, m_max, d = A.shape
            f.write(struct.pack("<5q", B, m_max, d, X.shape[-2], 1 if X.ndim == 2 else 0))
            for a, dt in ((A, np.float64), (b, np.float64), (np.full(B, m_max) if m is None else m, np.int32), (X, np.float64)):
                f.write(np.ascontiguousarray(a, dtype=dt).tobytes())


def run_program(exe, paths=()):
    return subprocess.run([exe] + list(paths), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)


# ---------------------------------------------------------------------------------------------------------- inputs
def unit_rows(A, b, m=None):
    """n = a / |a|, beta = b / |a|; a zero row (or one beyond m) -> n = 0, beta = 0 (b >= 0) or -1 (b < 0: empty)."""
    nrm = np.linalg.norm(A, axis=-1)
    z = nrm == 0
    s = np.where(z, 1.0, nrm)
    N, beta = A / s[..., None], np.where(z, np.where(b < 0, -1.0, 0.0), b / s)
    if m is not None:
        dead = np.arange(A.shape[-2]) >= np.asarray(m)[..., None]
        N, beta = np.where(dead[..., None], 0.0, N), np.where(dead, 0.0, beta)
    return N, beta


def points_for(O, A, b, m, seed, K_random=3):
    """Per polytope [B, K_random + 5, d]: standard normal x 3; a point inside (the Chebyshev centre); a point on a facet
    (from the centre along a random ray to the first row); a point in the normal cone of a vertex (the optimum of a random
    LP + a positive combination of the rows tight there); a point 1e3 extents away; a NaN.  A polytope without a centre
    or a vertex gets random points in those places.  Also -> centre[B, d] (NaN where there is none)."""
    B, _, d = A.shape
    rng = np.random.default_rng(seed)
    X = 3.0 * rng.standard_normal((B, K_random + 5, d))
    xc = np.full((B, d), np.nan)
    for p in range(B):
        mp = int(m[p])
        Ap, bp = A[p, :mp], b[p, :mp]
        if mp == 0:
            continue
        st, r, c = O.cheby(Ap, bp)
        if st == 0 and 0 < r < np.inf:
            xc[p] = c
            X[p, K_random] = c
            ray = rng.standard_normal(d)
            ar = Ap @ ray
            hit = ar > 1e-12
            if hit.any():
                X[p, K_random + 1] = c + np.min((bp - Ap @ c)[hit] / ar[hit]) * ray
            ext = max(1.0, float(np.max(np.abs(c))) + r)
        else:
            ext = 1.0
        st, xv, _, _ = O.lp_solve(rng.standard_normal(d), Ap, bp)
        if st == 0:
            tight = np.abs(Ap @ xv - bp) <= 1e-9 * max(1.0, float(np.max(np.abs(xv))))
            X[p, K_random + 2] = xv + (rng.random(int(tight.sum())) + 0.1) @ Ap[tight]
        far = rng.standard_normal(d)
        X[p, K_random + 3] = 1e3 * ext * far / np.linalg.norm(far)
    X[:, K_random + 4] = np.nan
    return X, xc


def _subsets(R, d):
    return [np.array(list(itertools.combinations(range(R), s)), dtype=np.int64).reshape(math.comb(R, s), s)
            for s in range(0, min(R, d) + 1)]


def reference(A, b, m, X, xfeas, empty=None):
    """-> dist[B, K], x[B, K, d], found bool[B, K] (False: no feasible candidate, or the point is not finite).
    xfeas[B, d]: a feasible point per polytope or NaN (then every row is a candidate).  empty bool[B]: polytopes the
    oracle's Chebyshev LP calls infeasible -- they are not enumerated and come back as not found."""
    B, m_max, d = A.shape
    Xb = np.broadcast_to(X, (B,) + X.shape) if X.ndim == 2 else X
    K = Xb.shape[1]
    N, beta = unit_rows(A, b, m)
    dist, xo, found = np.full((B, K), np.nan), np.full((B, K, d), np.nan), np.zeros((B, K), bool)
    P = Xb.reshape(B * K, d)
    pi = np.repeat(np.arange(B), K)
    fin = np.isfinite(P).all(axis=1)
    slack = np.where(fin[:, None], beta[pi] - np.einsum("qik,qk->qi", N[pi], np.where(fin[:, None], P, 0.0)), np.inf)
    live = (np.arange(m_max)[None, :] < np.asarray(m)[pi][:, None]) & ((np.abs(N[pi]).sum(axis=2) > 0) | (beta[pi] < 0))
    # Which rows can be active.  Hildreth's dual coordinate ascent (a fixed number of sweeps) gives multipliers lam >= 0,
    # whose dual value is a LOWER bound of f* = dist*^2 / 2 whatever they are, and a point xh; xh pulled towards the feasible
    # point until no row is violated is a feasible xf.  Strong convexity: |xf - x*|^2 / 2 <= f(xf) - f* <= f(xf) - dual =: g,
    # so a row active at x* has slack at xf of at most rho = sqrt(2 g) (a little is added: xfeas may be 1e-9 outside a row).
    Nq, bq_ = N[pi], beta[pi]
    P0 = np.where(fin[:, None], P, 0.0)
    lamh, xh = np.zeros((B * K, m_max)), P0.copy()
    for _ in range(HILDRETH_SWEEPS):
        for i in range(m_max):
            new = np.maximum(0.0, lamh[:, i] + np.einsum("qk,qk->q", Nq[:, i], xh) - bq_[:, i])
            xh -= (new - lamh[:, i])[:, None] * Nq[:, i]
            lamh[:, i] = new
    dual = -0.5 * np.sum((P0 - xh) ** 2, axis=1) + np.einsum("qi,qi->q", lamh, np.einsum("qik,qk->qi", Nq, P0) - bq_)
    has = fin & np.isfinite(xfeas[pi]).all(axis=1)
    x0 = np.where(has[:, None], xfeas[pi], 0.0)
    s0 = bq_ - np.einsum("qik,qk->qi", Nq, x0)
    ad = np.einsum("qik,qk->qi", Nq, xh - x0)
    with np.errstate(divide="ignore", invalid="ignore"):
        t = np.where(ad > 0, np.maximum(s0, 0.0) / ad, np.inf).min(axis=1, initial=1.0)
    xf = x0 + np.clip(t, 0.0, 1.0)[:, None] * (xh - x0)
    rho = np.sqrt(np.maximum(0.0, 2.0 * (0.5 * np.sum((xf - P0) ** 2, axis=1) - dual)))
    Ef = np.maximum(1.0, np.abs(xf).max(axis=1, initial=0.0))
    has &= (s0 >= -1e-8 * Ef[:, None]).all(axis=1)
    sf = bq_ - np.einsum("qik,qk->qi", Nq, xf)
    cand = live & (~has[:, None] | (sf <= (rho + 1e-6 * Ef)[:, None]))
    if empty is not None:   # (the oracle's verdict is taken: nothing is enumerated for an empty polytope)
        fin = fin & ~np.asarray(empty)[pi]
    cnt = cand.sum(axis=1)
    E = np.maximum(1.0, np.abs(np.where(fin[:, None], P, 0.0)).max(axis=1, initial=0.0))
    flat_d, flat_x, flat_f = dist.reshape(-1), xo.reshape(-1, d), found.reshape(-1)
    sizes = (4, 6, 8, 10, 12, 14, 16, 18, 20, 22, 24, 28, 32, 40, 48, 64)
    for lo, R in zip((-1,) + sizes, sizes):
        sel = np.nonzero(fin & (cnt > lo) & (cnt <= R))[0]
        R = min(R, m_max)
        if not sel.size:
            continue
        subs = _subsets(R, d)
        chunk = max(1, int(2e6 // max(1, sum(len(s) for s in subs))))
        for c0 in range(0, sel.size, chunk):
            q = sel[c0:c0 + chunk]
            # the R rows of least slack (candidates first); rows that are no candidates are made zero rows
            order = np.argsort(np.where(cand[q], slack[q], np.inf), axis=1, kind="stable")[:, :R]
            keep = np.take_along_axis(cand[q], order, axis=1)
            Nq = np.take_along_axis(N[pi[q]], order[:, :, None], axis=1) * keep[:, :, None]
            bq = np.take_along_axis(beta[pi[q]], order, axis=1) * keep
            best = np.full(q.size, np.inf)
            bx = np.full((q.size, d), np.nan)
            Nall, ball, pall = N[pi[q]], beta[pi[q]], P[q]
            for S in subs:
                if S.shape[1] == 0:
                    xs = pall[:, None, :]
                else:
                    NS, bS = Nq[:, S], bq[:, S]                     # [Q, nsub, s, d], [Q, nsub, s]
                    res = np.einsum("qnsk,qk->qns", NS, pall) - bS
                    xs = pall[:, None, :] - np.einsum("qnks,qns->qnk", np.linalg.pinv(NS), res)
                viol = (np.einsum("qik,qnk->qni", Nall, xs) - ball[:, None, :]).max(axis=2, initial=-np.inf)
                En = np.maximum(E[q][:, None], np.abs(xs).max(axis=2))
                dd = np.where(viol <= REF_FEAS * En, np.linalg.norm(xs - pall[:, None, :], axis=2), np.inf)
                j = dd.argmin(axis=1)
                dj = dd[np.arange(q.size), j]
                up = dj < best
                best = np.where(up, dj, best)
                bx[up] = xs[np.arange(q.size), j][up]
            ok = np.isfinite(best)
            flat_d[q[ok]], flat_x[q[ok]], flat_f[q[ok]] = best[ok], bx[ok], True
    return dist, xo, found


def exact_reference(A, b, p):
    """The nearest point of { A x <= b } to p in EXACT rational arithmetic on the doubles as stored: every independent
    subset of at most d rows, x = p - A_S' (A_S A_S')^-1 (A_S p - b_S), the feasible ones, the least |x - p|^2.
    -> (dist as a float, x as Fractions), or (None, None) when no candidate is feasible (the set is empty)."""
    from fractions import Fraction as F
    A = [[F(float(v)) for v in row] for row in np.asarray(A)]
    b = [F(float(v)) for v in np.asarray(b)]
    p = [F(float(v)) for v in p]
    m, d = len(A), len(p)
    live = [i for i in range(m) if any(A[i]) or b[i] < 0]
    if any(not any(A[i]) for i in live):
        return None, None
    res = [sum(A[i][k] * p[k] for k in range(d)) - b[i] for i in range(m)]
    G = [[sum(A[i][k] * A[j][k] for k in range(d)) for j in range(m)] for i in range(m)]
    best, bx = None, None
    for s in range(0, min(d, len(live)) + 1):
        for S in itertools.combinations(live, s):
            M = [[G[i][j] for j in S] + [res[i]] for i in S]
            sing = False
            for c in range(s):   # Gauss-Jordan
                piv = next((r for r in range(c, s) if M[r][c] != 0), None)
                if piv is None:
                    sing = True
                    break
                M[c], M[piv] = M[piv], M[c]
                M[c] = [v / M[c][c] for v in M[c]]
                for r in range(s):
                    if r != c and M[r][c] != 0:
                        f = M[r][c]
                        M[r] = [vr - f * vc for vr, vc in zip(M[r], M[c])]
            if sing:
                continue
            x = [p[k] - sum(M[a][s] * A[i][k] for a, i in enumerate(S)) for k in range(d)]
            d2 = sum((x[k] - p[k]) ** 2 for k in range(d))
            if best is not None and d2 >= best:
                continue
            if all(sum(A[i][k] * x[k] for k in range(d)) <= b[i] for i in live):
                best, bx = d2, x
    if best is None:
        return None, None
    return math.sqrt(float(best)), bx


# ---------------------------------------------------------------------------------------------------------- cases
def _case(O, A, b, m, seed):
    X, xc = points_for(O, A, b, m, seed)
    Xs = X[0].copy()   # the points of polytope 0, shared by all
    case = {"shape": A.shape[1:], "A": A, "b": b, "m": m, "xc": xc}
    # the oracle's verdict, read as cheby_ball reads the LP: infeasible, or a radius below zero (by more than rounding)
    balls = [O.cheby(A[p, :m[p]], b[p, :m[p]])[:2] if m[p] else (0, np.inf) for p in range(A.shape[0])]
    empty = np.array([st == 2 or (st == 0 and r < -1e-12) for st, r in balls])
    case["oracle_empty"] = empty
    for name, P in (("shared", Xs), ("own", X)):
        case[name] = (P,) + reference(A, b, m, P, xc, empty)
    return case


def soak_cases(O, fam, seed, shapes=SOAK_SHAPES, B=B_CPU):
    """Per shape the polytopes of soak family `fam` (one generator carried through the shapes, as support_host.soak_cases)
    with points_for's points: per polytope ("own", [B, 8, d]) and those of polytope 0 for all ("shared", [8, d]); the
    reference's answers; the oracle's Chebyshev verdict."""
    rng = np.random.default_rng(seed)
    out = []
    for s, (m_max, d) in enumerate(shapes):
        A, b, m = sh.family(fam, B=B, rng=rng, shape=(m_max, d))
        out.append(_case(O, A, b, m, [seed, s, 91]))
    return out


def degenerate_cases(O):
    """The polytopes support_host.degenerate_cases draws on (pyramids, the structured (16, 3) polytopes, the degenerate LPs'
    polytopes at d <= 4) and three by hand: an empty set, a single point, m = 0."""
    out = []
    for s, c in enumerate(sh.memo(("degenerate",), lambda: sh.degenerate_cases(O))):
        out.append(_case(O, c["A"][:B_CPU], c["b"][:B_CPU], c["m"][:B_CPU], [4243, s]))   # (the first B_CPU of each batch)
    out.append(hand_case(O))
    return out


def hand_case(O):
    """Four polytopes by hand at (8, 3): an empty set, a single point, m = 0, a zero row with b < 0."""
    d = 3
    box = np.vstack([np.eye(d), -np.eye(d)])
    A = np.zeros((4, 8, d))
    b = np.zeros((4, 8))
    A[:, :6], b[:, :6] = box, 1.0
    A[0, 6], b[0, 6] = [1.0, 1.0, 0.0], -3.0            # empty: x + y <= -3 inside the unit box
    b[1, :6] = [0.5, 0.25, 0.0, -0.5, -0.25, 0.0]       # the single point (0.5, 0.25, 0)
    b[3, 7] = -1.0                                      # a zero row with b < 0: empty by that row alone
    m = np.array([7, 6, 0, 8], np.int32)
    return _case(O, A, b, m, [4243, 99])


def random_cases(O):
    """support_host.family(k): random_hpolytopes, ragged, at SHAPES, the first B_CPU of each."""
    out = []
    for k in range(len(sh.SHAPES)):
        A, b, m = sh.family(k)
        out.append(_case(O, A[:B_CPU], b[:B_CPU], m[:B_CPU], [sh.SEED0, k, 92]))
    return out


def cases(O, fam):
    if fam == "degenerate":
        return sh.memo(("nearest", "degenerate"), lambda: degenerate_cases(O))
    if fam == "family":
        return sh.memo(("nearest", "family"), lambda: random_cases(O))
    return sh.memo(("nearest", fam), lambda: soak_cases(O, fam, sh.FAMILY_SEED[fam]))


# ---------------------------------------------------------------------------------------------------------- checks
def certificate(N, beta, p, x, face, lam_given, nrm):
    """The kernel's optimality certificate recomputed from face and lam: (gap, |r|_2) with lam_j |a_j| on the unit rows."""
    rows = [i for i in range(64) if (int(face) >> i) & 1]
    lam = np.array([lam_given[j] * nrm[i] for j, i in enumerate(rows)])
    gap = float(np.sum(lam * np.abs(beta[rows] - N[rows] @ x))) if rows else 0.0
    r = (p - x) - (lam @ N[rows] if rows else 0.0)
    return gap, float(np.linalg.norm(r)), lam


def check_case(case, layout, out, counts=None, separated=False, resolved=False):
    """What every status-0 answer must satisfy (the module docstring of tests/test_nearest_host.py), and what the statuses
    may be.  counts: [problems with a finite point, handed back among them] is added to."""
    A, b, m = case["A"], case["b"], case["m"]
    P, rd, rx, rfound = case[layout]
    B, _, d = A.shape
    Pb = np.broadcast_to(P, (B,) + P.shape) if P.ndim == 2 else P
    N, beta = unit_rows(A, b, m)
    nrm = np.linalg.norm(A, axis=-1)
    st, dist, x, face, lam = out["status"], out["dist"], out["x"], out["face"], out["lam"]
    fin = np.isfinite(Pb).all(axis=2)
    assert set(np.unique(st).tolist()) <= ({0, 2, 4} if resolved else {0, 1, 2})
    assert np.all(st[~fin] == (4 if resolved else 1))
    assert np.all(np.isnan(dist[st != 0])) and (x is None or np.all(np.isnan(x[st != 0])))
    # status 2 only where the reference finds no feasible candidate and the oracle's Chebyshev LP says infeasible; never 0 there
    empty = case["oracle_empty"][:, None] & ~rfound
    assert not np.any((st == 2) & ~empty), np.argwhere((st == 2) & ~empty)[:5]
    assert not np.any((st == 0) & ~rfound & fin), np.argwhere((st == 0) & ~rfound & fin)[:5]
    if resolved:
        assert np.all(st[rfound] == 0)
    for p_, j in np.argwhere(st == 0):
        pt, xx = Pb[p_, j], x[p_, j]
        E = max(1.0, float(np.max(np.abs(xx))), float(np.max(np.abs(pt))))
        assert np.max(N[p_] @ xx - beta[p_], initial=-np.inf) <= TOL * E, (p_, j)
        nd = float(np.linalg.norm(xx - pt))
        assert abs(dist[p_, j] - nd) <= 1e-12 * max(nd, 1e-300) or nd == dist[p_, j], (p_, j, dist[p_, j], nd)
        assert abs(dist[p_, j] - rd[p_, j]) <= TOL * E, (p_, j, dist[p_, j], rd[p_, j])
        if separated:
            assert np.max(np.abs(xx - rx[p_, j])) <= TOL * E, (p_, j, xx, rx[p_, j])
        if face is not None:
            gap, r2, l = certificate(N[p_], beta[p_], pt, xx, face[p_, j], lam[p_, j], nrm[p_])
            assert np.all(l >= 0) and bin(int(face[p_, j])).count("1") <= d and int(face[p_, j]) >> int(m[p_]) == 0
            assert gap <= 1e-10 * E * max(nd, 1e-10 * E) * (1 + 1e-6) and r2 <= 1e-12 * E * (1 + 1e-6), (p_, j, gap, r2)
            assert np.all(lam[p_, j, len(l):] == 0)
            if nd == 0:
                assert np.array_equal(xx, pt)
    if counts is not None:
        counts[0] += int(fin.sum())
        counts[1] += int((st[fin] == 1).sum())
