"""What tests/test_batch_contract_host.py (CPU) and tests/test_batch_contract_gpu.py share: the packed-table contract of
include/plp.h -- rows from m[p] on, points from n[p] on, rows or points whose keep bit is clear and rows of Q beyond mq[p]
do not exist, and member p's answer depends on member p only -- as inputs that make a violation visible.

poison()          the padding of a packed table overwritten with NaN, 1e300 or values that would change the answer;
exact_hull()      the facets of a point set and exact_vertices() the vertices of {A x <= b}, both in rational arithmetic
                  over all d-subsets, with the smallest non-zero distance met on the way (so a test can show that the
                  tolerant rule of the kernel and the exact rule cannot disagree on its input);
lattice_sets()    the inputs of those two: small integers, many points per face, exact repeats, flat sets, empty
integer_polytopes()  polytopes.
Helpers only: no tests here."""
import itertools
import math
from fractions import Fraction

import numpy as np

from extreme_host import XS_EMPTY, XS_OK
from hull_host import HS_FLAT, HS_OK

KINDS = ("zero", "nan", "huge", "cut")
HUGE = 1e300            # finite, but its square is inf: a norm or a box taken over the padding shows
MIN_DISTANCE = 1e-6     # a thousand times the kernels' 1e-9: what every exact case has to keep clear of
HULL_CASES = {2: 25, 3: 25, 4: 25}       # exact cases per dimension, sized by what the rational arithmetic costs: every
VERTEX_CASES = {2: 25, 3: 25, 4: 6}      # d-subset of up to 16 rows at d = 4 is a 4 x 4 system solved five times over


# ------------------------------------------------------------------------------------------------ poison
def _dead(m, slots, keep):
    """bool[B, slots]: slot i of member p does not exist (i >= m[p], or bit i of keep[p] -- [B] or [B, W] words -- clear)."""
    m = np.asarray(m).astype(np.int64)
    idx = np.arange(slots)
    dead = idx[None, :] >= m[:, None]
    if keep is not None:
        words = np.ascontiguousarray(keep).view(np.uint64).reshape(m.shape[0], -1)
        bit = (words[:, idx // 64] >> (idx % 64).astype(np.uint64)[None, :]) & np.uint64(1)
        dead |= bit == 0
    return dead


def poison(arrays, m, kind, keep=None, what="rows", violated_by=None):
    """Copies of `arrays` with everything that does not exist overwritten.
    what = "rows":   arrays = (A[B, m_max, d], b[B, m_max]);
    what = "points": arrays = (X[B, n_max, d],);
    what = "q":      arrays = (QA[B, mq_max, d], Qb[B, mq_max]), m = mq, violated_by[B, d] a point of each P.
    kind: "zero" (the baseline), "nan", "huge" (1e300) or "cut": finite, plausible and answer-changing --
      rows:   a copy of live row 0 with b lowered by 10 x the extent of the polytope (max(1, |b_i| / |a_i|) over its live
              rows), which leaves nothing of it; without a live row, x_0 <= -10;
      points: points 1e3 x the extent of the set (max(1, |x|) over its live points) away from it, each in an orthant of
              its own where there are enough: they would all be vertices;
      q:      the row x_0 <= violated_by_0 - 1, which P violates.
    (The boxes of plp_volume_hits have no padding: lb / ub are not touched by any kind.)"""
    assert kind in KINDS and what in ("rows", "points", "q")
    out = [np.array(a, dtype=np.float64, copy=True) for a in arrays]
    lead = out[0]
    B, slots, d = lead.shape
    dead = _dead(m, slots, keep)
    if kind != "cut":
        v = {"zero": 0.0, "nan": np.nan, "huge": HUGE}[kind]
        for a in out:
            a[dead] = v
        return out
    if what == "rows":   # (vectorised: the large batches of the GPU tests come through here)
        A, b = out
        alive = ~dead
        has = alive.any(axis=1)
        first = np.argmax(alive, axis=1)
        nrm = np.linalg.norm(A, axis=2)
        ratio = np.where(alive, np.abs(b) / np.where(nrm > 0, nrm, 1.0), 0.0)
        ext = np.maximum(1.0, ratio.max(axis=1))
        row, rhs = A[np.arange(B), first].copy(), b[np.arange(B), first].copy()
        none = ~has | ~row.any(axis=1)
        row[none] = np.eye(d)[0]
        rhs = np.where(has, rhs - 10.0 * ext * np.maximum(1.0, np.linalg.norm(row, axis=1)), -10.0)
        A[dead] = np.broadcast_to(row[:, None, :], A.shape)[dead]
        b[dead] = np.broadcast_to(rhs[:, None], b.shape)[dead]
        return out
    for p in range(B):
        holes = np.nonzero(dead[p])[0]
        if holes.size == 0:
            continue
        live = np.nonzero(~dead[p])[0]
        if what == "points":
            X = out[0]
            ext = max(1.0, float(np.max(np.abs(X[p, live])))) if live.size else 1.0
            for t, i in enumerate(holes):
                sign = np.array([1.0 if (t >> k) & 1 else -1.0 for k in range(d)])
                X[p, i] = 1e3 * ext * (1.0 + t // (1 << d)) * sign
        else:
            QA, Qb = out
            QA[p, holes] = np.eye(d)[0]
            Qb[p, holes] = violated_by[p, 0] - 1.0
    return out


# ------------------------------------------------------------------------------------------------ exact references
def _exact(v):
    """A double as the rational number it is (an int where it is integral: the same arithmetic, only faster)."""
    v = float(v)
    return int(v) if v == int(v) else Fraction(v)


def _frac(a):
    return [[_exact(v) for v in row] for row in np.asarray(a, dtype=np.float64)]


def _det(M):
    """Determinant of a small square matrix of Fractions (cofactors along the first row)."""
    n = len(M)
    if n == 1:
        return M[0][0]
    if n == 2:
        return M[0][0] * M[1][1] - M[0][1] * M[1][0]
    return sum((-1) ** j * M[0][j] * _det([row[:j] + row[j + 1:] for row in M[1:]]) for j in range(n) if M[0][j] != 0)


def _normal(edges, d):
    """The generalised cross product of d - 1 edges in R^d (d = 1: (1))."""
    if d == 1:
        return [1]
    return [(-1) ** k * _det([e[:k] + e[k + 1:] for e in edges]) for k in range(d)]


def exact_hull(points):
    """The convex hull of points[n, d] in exact rational arithmetic, every d-subset a candidate plane
    -> (facets, least): facets = the set of frozensets of the indices of the points on each facet, or None for a flat set
    (fewer than d + 1 points, or all in one hyperplane); least = the smallest non-zero value met of what the kernel holds
    against a tolerance, on its own scaling (points moved to the centre of their box and divided by the largest |p - c|_inf):
    the distance of a point from a candidate plane, and |nu| / prod |edges| of a subset in general position.  inf when
    nothing non-zero was met."""
    P = _frac(points)
    n = len(P)
    d = len(P[0]) if n else np.asarray(points).shape[-1]
    least = math.inf
    if n < d + 1:
        return None, least
    c = [Fraction(min(p[k] for p in P) + max(p[k] for p in P)) / 2 for k in range(d)]
    s = max(abs(p[k] - c[k]) for p in P for k in range(d))
    if s == 0:
        return None, least
    facets, flat, any_plane = set(), False, False
    for S in itertools.combinations(range(n), d):
        edges = [[P[i][k] - P[S[0]][k] for k in range(d)] for i in S[1:]]
        nu = _normal(edges, d)
        nn2 = sum(v * v for v in nu)
        if nn2 == 0:
            continue
        any_plane = True
        nn = math.sqrt(float(nn2))
        least = min(least, nn / math.prod(math.sqrt(float(sum(v * v for v in e))) for e in edges))
        r = [sum(nu[k] * (p[k] - P[S[0]][k]) for k in range(d)) for p in P]
        for v in r:
            if v != 0:
                least = min(least, abs(float(v)) / (nn * float(s)))
        hi, lo = max(r), min(r)
        if hi == 0 and lo == 0:
            flat = True
            break
        if hi == 0 or lo == 0:
            facets.add(frozenset(i for i in range(n) if r[i] == 0))
    if flat or not any_plane:
        return None, least
    return facets, least


def _solve(M, rhs):
    """M x = rhs by Cramer's rule -> (x as Fractions, det) or (None, 0) for a singular M."""
    det = _det(M)
    if det == 0:
        return None, 0
    n = len(M)
    return [Fraction(_det([row[:k] + [rhs[i]] + row[k + 1:] for i, row in enumerate(M)])) / det for k in range(n)], det


def exact_vertices(A, b):
    """The vertices of {A x <= b} (A[m, d], b[m]) in exact rational arithmetic, every d-subset of the rows a candidate
    -> (vertices, least): vertices = the set of tuples of Fractions (empty: no subset gives a feasible point, or a zero row
    with b < 0); least = the smallest non-zero value met of what the kernel holds against a tolerance, on its own scaling
    (rows of unit 2-norm): |det| of a subset, the distance of a candidate from a row over max(1, |v|_inf, |b_i| / |a_i|),
    and the distance of two vertices in the max-norm over max(1, |v|_inf) of the larger.  inf when nothing non-zero was
    met."""
    rows, rhs = _frac(A), [_exact(v) for v in np.asarray(b, dtype=np.float64)]
    least = math.inf
    d = len(rows[0]) if rows else np.asarray(A).shape[-1]
    live = []
    for a, beta in zip(rows, rhs):
        if all(v == 0 for v in a):
            if beta < 0:
                return set(), least
            continue
        live.append((a, beta, math.sqrt(float(sum(v * v for v in a)))))
    verts = set()
    for S in itertools.combinations(range(len(live)), d):
        v, det = _solve([live[i][0] for i in S], [live[i][1] for i in S])
        if v is None:
            continue
        least = min(least, abs(float(det)) / math.prod(live[i][2] for i in S))
        vn = max(1.0, max(abs(float(t)) for t in v))
        ok = True
        for a, beta, nrm in live:
            slack = sum(a[k] * v[k] for k in range(d)) - beta
            if slack != 0:
                least = min(least, abs(float(slack)) / nrm / max(vn, abs(float(beta)) / nrm))
            ok = ok and slack <= 0
        if ok:
            verts.add(tuple(v))
    for v, w in itertools.combinations(verts, 2):
        dist = max(abs(float(x - y)) for x, y in zip(v, w))
        least = min(least, dist / max(1.0, max(abs(float(t)) for t in v + w)))
    return verts, least


# ------------------------------------------------------------------------------------------------ generators
def lattice_sets(d, count, seed):
    """`count` point sets in Z^d: n = 9 .. 14 points with coordinates in -2 .. 2 (faces that carry many points, and in the
    plane exact repeats by themselves).  Forced: case 1 repeats a point exactly, case 2 is flat (its last coordinate
    constant), case 3 has fewer than d + 1 points.  -> a list of float arrays [n, d]."""
    rng = np.random.default_rng(seed)
    out = []
    for t in range(count):
        n = int(rng.integers(9, 15))
        X = rng.integers(-2, 3, (n, d)).astype(np.float64)
        if t == 1:
            X[n - 1] = X[0]
            X[4] = X[0]
        elif t == 2:
            X[:, -1] = 1.0
        elif t == 3:
            X = X[:d]
        out.append(X)
    return out


def integer_polytopes(d, count, seed):
    """`count` polytopes with integer rows: the box |x_i| <= 2 plus 2 .. 6 rows with entries in -3 .. 3 and b in 0 .. 4 (the
    origin is inside; up to a few dozen vertices, many of them on more than d rows).  Forced: case 1 repeats a row
    exactly, case 2 is flat (x_0 <= 1 and -x_0 <= -1: it still has vertices), cases 3 and 4 are empty (x_0 <= -3 against
    the box; a zero row with b = -1).  -> a list of (A[m, d], b[m]) float arrays."""
    rng = np.random.default_rng(seed)
    out = []
    for t in range(count):
        k = int(rng.integers(2, 7))
        R = rng.integers(-3, 4, (k, d))
        R[np.all(R == 0, axis=1), 0] = 1
        A = np.vstack([np.eye(d), -np.eye(d), R]).astype(np.float64)
        b = np.hstack([np.full(2 * d, 2.0), rng.integers(0, 5, k).astype(np.float64)])
        if t == 1:
            A, b = np.vstack([A, A[2 * d]]), np.hstack([b, b[2 * d]])
        elif t == 2:
            A = np.vstack([A, np.eye(d)[0], -np.eye(d)[0]])
            b = np.hstack([b, 1.0, -1.0])
        elif t == 3:
            A, b = np.vstack([A, np.eye(d)[0]]), np.hstack([b, -3.0])
        elif t == 4:
            A, b = np.vstack([A, np.zeros(d)]), np.hstack([b, -1.0])
        perm = rng.permutation(len(b))
        out.append((A[perm], b[perm]))
    return out


def pack_rows(cases):
    """[(A, b)] of one dimension -> A[B, m_max, d], b[B, m_max], m[B], zero padded."""
    d = cases[0][0].shape[1]
    m = np.array([len(bb) for _, bb in cases], np.int32)
    A = np.zeros((len(cases), int(m.max()), d))
    b = np.zeros((len(cases), int(m.max())))
    for k, (Ak, bk) in enumerate(cases):
        A[k, :m[k]], b[k, :m[k]] = Ak, bk
    return A, b, m


def pack_points(sets):
    """[X] of one dimension -> X[B, n_max, d], n[B], zero padded."""
    d = sets[0].shape[1]
    n = np.array([len(X) for X in sets], np.int32)
    out = np.zeros((len(sets), int(n.max()), d))
    for k, X in enumerate(sets):
        out[k, :n[k]] = X
    return out, n


# ------------------------------------------------------------------------------------------------ the two comparisons
def check_hull(points, A, b, on, count, status, side_tol=1e-9):
    """One hull result (rows A[f_max, d], b[f_max], incidence words on[f_max], count, status of plp_hull_batch's rule)
    against exact_hull(points): status, count and the set of incidence words equal; each written row a unit normal with
    |a.x_i - b| <= side_tol E on its incident points (E = the extent the rule scales by: the largest |x - c|_inf from the
    centre c of the box of the set) and a.x_i <= b + side_tol E on all.
    -> least (the caller holds it against MIN_DISTANCE)."""
    facets, least = exact_hull(points)
    if facets is None:
        assert status == HS_FLAT and count == 0, (status, count)
        return least
    assert status == HS_OK and count == len(facets), (status, count, len(facets))
    words = [int(w) for w in np.ascontiguousarray(on[:count]).view(np.uint64)]
    got = {frozenset(i for i in range(64) if (w >> i) & 1) for w in words}
    assert len(got) == count and got == facets, (sorted(map(sorted, got)), sorted(map(sorted, facets)))
    X = np.asarray(points, dtype=np.float64)
    c = (X.min(axis=0) + X.max(axis=0)) / 2
    E = float(np.max(np.abs(X - c)))
    for q in range(count):
        assert abs(float(np.linalg.norm(A[q])) - 1.0) <= 1e-12
        r = X @ A[q] - b[q]
        inc = [i for i in range(len(X)) if (words[q] >> i) & 1]
        assert np.all(np.abs(r[inc]) <= side_tol * E) and np.all(r <= side_tol * E), (q, r)
    return least


def check_vertices(A, b, V, count, status, match):
    """One vertex list (V[v_max, d], count, status of plp_extreme_batch's rule) against exact_vertices(A, b): status and
    count equal; every vertex within match max(1, |v|_inf) of an exact one and every exact one of a written one.
    -> least."""
    verts, least = exact_vertices(A, b)
    if not verts:
        assert status == XS_EMPTY and count == 0, (status, count)
        return least
    assert status == XS_OK and count == len(verts), (status, count, len(verts))
    W = np.array([[float(t) for t in v] for v in verts])
    G = np.asarray(V[:count], dtype=np.float64)
    assert np.all(np.isfinite(G))
    for v in G:
        assert np.min(np.max(np.abs(W - v), axis=1)) <= match * max(1.0, float(np.max(np.abs(v)))), v
    for w in W:
        assert np.min(np.max(np.abs(G - w), axis=1)) <= match * max(1.0, float(np.max(np.abs(w)))), w
    return least


# ------------------------------------------------------------------------------------------------ mixed batches
def keep_words(rng, B, forced, share=0.8):
    """uint64[B] keep words with holes: bit i set with probability `share`, the first `forced` bits always; member 0
    keeps everything."""
    keep = np.zeros(B, np.uint64)
    for p in range(B):
        mask = rng.random(64) < share
        mask[:min(forced, 64)] = True
        keep[p] = np.uint64(sum(1 << int(i) for i in np.nonzero(mask)[0]))
    keep[0] = np.uint64(2 ** 64 - 1)
    return keep


def mixed_rows(B, m_max, d, seed, min_m=0, bounded_only=False):
    """B ragged polytopes with the origin strictly inside where they have an inside at all: unit rows tangent to spheres of
    radius 1 .. 2, the first 2 d rows the box |x_i| <= 3 where there is room for it.  No two rows tie in a ratio test
    (random data).  Member 0 uses all m_max rows, and with B >= 5 (unless bounded_only):
      member 1 has m = min_m rows, member 2 is unbounded (d random rows, no box), member 3 is empty (row 1 = -row 0 with
      b_1 = -b_0 - 1), member 4 is flat and not empty (a random row and its negative through the origin, behind the box
      where there is room for both);
    every other member has 2 d + 1 .. m_max rows (d + 1 .. m_max without room for the box).  B = 1: one row short of m_max,
    so that there is padding.  Padding is zero.  -> A[B, m_max, d], b[B, m_max], m int32[B]."""
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((B, m_max, d))
    A /= np.linalg.norm(A, axis=2, keepdims=True)
    b = 1.0 + rng.random((B, m_max))
    box = m_max >= 2 * d
    if box:
        A[:, :2 * d] = np.vstack([np.eye(d), -np.eye(d)])[None]
        b[:, :2 * d] = 3.0
    lo = min(m_max, 2 * d + 1 if box else d + 1)
    m = rng.integers(lo, m_max + 1, size=B).astype(np.int32)
    m[0] = m_max if B > 1 else max(min(lo, m_max), m_max - 1)
    if B >= 5 and not bounded_only:
        m[1] = min_m
        m[2] = min(d, m_max)
        A[2, :m[2]] = rng.standard_normal((m[2], d))
        A[2, :m[2]] /= np.linalg.norm(A[2, :m[2]], axis=1, keepdims=True)
        b[2, :m[2]] = 1.0 + rng.random(m[2])
        A[3, 1], b[3, 1] = -A[3, 0], -b[3, 0] - 1.0
        j = 2 * d if box and m_max >= 2 * d + 2 else 0
        A[4, j + 1], b[4, j], b[4, j + 1] = -A[4, j], 0.0, 0.0
        m[4] = max(m[4], j + 2)
    pad = np.arange(m_max)[None, :] >= m[:, None]
    A[pad], b[pad] = 0.0, 0.0
    return A, b, m


def mixed_points(B, n_max, d, seed):
    """B ragged point sets at three scales and away from the origin.  Member 0 uses all n_max points, and with B >= 5:
    member 1 has no point, member 2 has d points (too few), member 3 is flat (last coordinate constant), member 4 is a
    lattice set (integers in -2 .. 2: faces with many points); every other member has d + 1 .. n_max points, an exact
    repeat of point 0 in every second one.  Padding is zero.  -> X[B, n_max, d], n int32[B]."""
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((B, n_max, d)) * rng.choice([1.0, 1e-2, 1e3], size=(B, 1, 1)) + 3.0 * rng.standard_normal((B, 1, d))
    lo = min(n_max, d + 1)
    n = rng.integers(lo, n_max + 1, size=B).astype(np.int32)
    n[0] = n_max if B > 1 else max(lo, n_max - 1)
    for p in range(B):
        if p % 2 and n[p] > 3:
            X[p, 3] = X[p, 0]
    if B >= 5:
        n[1] = 0
        n[2] = min(d, n_max)
        X[3, :, -1] = 0.25
        X[4] = rng.integers(-2, 3, (n_max, d)).astype(np.float64)
    for p in range(B):
        X[p, n[p]:] = 0.0
    return X, n


def same_bits(a, b):
    """Two arrays equal bit for bit (NaN compares as its bits)."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype.itemsize != b.dtype.itemsize:
        return False
    return bool(np.array_equal(a.view(np.uint8), b.view(np.uint8)))
