"""Polytope / Region and the set operations on the LP hot path -- host-side mirror of the
reference's public interface for that path (polytope/polytope.py of tulip-control/polytope).

Same names, argument meaning, caches and error behaviour as the reference; the difference is
where the linear programs go.  Wherever the reference issues LPs one at a time from a Python
loop, this module collects them and issues ONE batched call into the HIP engine
(polytope_amd.batch) when `solvers.default_solver == 'hip'`:

    cheby_ball / is_fulldim     1 LP (F1) per polytope; Regions -> one batch      (ref :1241-1300, :962-985)
    bounding_box                2d LPs (F3) -> one batch                           (ref :1314-1411)
    reduce                      fused kernel: F1 + dedupe + 2d F3 + m F2           (ref :1053-1163)
    Region.intersect            all pair stacks reduced in one batch               (ref :815-830)
    region_diff                 pre-scan, level scans, sibling nodes = one F1 batch each (ref :2117-2282)
    envelope                    all (facet, other polytope) F1 LPs in one batch    (ref :1414-1464)
    is_adjacent_pairs           all pair LPs in one batch                          (ref :1827-1866)
    contains                    dense kernel                                       (ref :206-218, :732-746)
    qhull / extreme             quickhull with device-resident outside sets        (ref :1597-1695, quickhull.py)

With any other backend name the LPs go through `solvers.lpsolve` one by one, as in the
reference.  There is no silent fallback between backends.

    projection (fm)             Fourier-Motzkin steps on the device, fused with the reduce   (ref :1698-1952)

Out of scope here: rotation, plotting, grid helpers; projection's "esp" solver (needs glpk).
"""
import logging
import warnings

import numpy as np

from . import solvers
from .solvers import lpsolve

logger = logging.getLogger(__name__)
_F64 = np.dtype(np.float64)

# global default absolute tolerance (module global so the magic methods can use it; ref :83)
ABS_TOL = 1e-7

# The reference's host flow has behaviours that are artefacts of its implementation rather than of the sets it computes with:
# `list.remove` takes out the first element that compares EQUAL, and Polytope.__eq__ is "both differences have a sampled volume
# below 1e-7" -- true between any two pieces that small, decided by an UNSEEDED random sample (ref :220-230, :1032-1050, :1586);
# subtrahends that do not touch a piece still pass it through copies, envelopes and reductions that move its numbers by an ulp,
# which later decides which of two coinciding rows a dedupe keeps.  With STRICT_REFERENCE_QUIRKS (the default) `union(check_convex)`
# and `mldivide(Region, Region)` replay them (_ref_index, _renormalised, _passed_untouched below) so that the fixtures generated
# from the reference are reproduced piece for piece, row for row; set it to False for the same SETS without the replay
# (pieces may come in another order / with rows in another order, tiny pieces are neither dropped nor doubled) and without its
# cost: Region(1000 cells).intersect(P) 41 -> 30 ms, is_subset(200 cells, 1000 cells) 18 -> 13 ms.
STRICT_REFERENCE_QUIRKS = True

_RF_EMPTY, _RF_EARLY, _RF_MINREP, _RF_LPFAIL = 1, 2, 4, 8
_RF_F1OPEN = 32   # empty because the fused kernel's Chebyshev LP did not end optimal, or ended outside the polytope (csrc/plp_common.hpp): re-examined below
_MAX_ROWS, _MAX_DIM = 64, 16
_RDIFF_NATIVE = True   # region_diff's search in the library (False: the host loop over batched calls, for A/B runs)


def _use_hip():
    return solvers.default_solver == "hip"


def _fits(m, d):
    """Fused reduce / bounding-box / containment kernels: register-resident dictionaries, m <= 64."""
    return 1 <= d <= _MAX_DIM and m <= _MAX_ROWS


def _max_rows_reduce(d):
    """Rows the fused reduce takes: up to 64 on the register-resident kernels, beyond that one polytope per wavefront
    with its rows and the dictionary of the LP being solved in LDS (csrc/plp_lds.hip: reduce_lds_kernel) -- what fits
    the CU's 160 KB (about 500 rows at d = 16, 2000 at d = 3)."""
    per_row = (((d + 1) | 1) * 8 + 24) + ((d + 4) * 8 + 4)
    return max(_MAX_ROWS, (160 * 1024 - 1400) // per_row)


def _fits_reduce(m, d):
    """reduce() on the 'hip' backend (the reference has no row limit: Polytope.intersect stacks m1 + m2 rows, ref
    :268-275, region_diff's leaves whatever the search collected, :2276)."""
    return 1 <= d <= _MAX_DIM and m <= _max_rows_reduce(d)


def _max_rows_lp(d):
    """Rows a stand-alone LP may have: beyond 64 the engine keeps the dictionary in LDS (csrc/plp_lds.hip), one LP
    per wavefront, and the limit is what fits the CU's 160 KB (d + 1 structural columns + the artificial one)."""
    return (160 * 1024 - 1024) // ((((d + 2) | 1) * 8) + 24)


def _fits_lp(m, d):
    """Chebyshev / generic LP batches (region_diff stacks m_poly + sum(active rows): ref :2212-2224 has no limit)."""
    return 1 <= d <= _MAX_DIM and m <= _max_rows_lp(d)


# ======================================================================================
class _NoDeviceState(object):
    """Objects that remember device-resident tables (`_packed`, `_p2p_flat`) pickle and deep-copy WITHOUT them: the
    copy packs its own table on first use, and a pickle opens on a host that has no GPU."""

    def __getstate__(self):
        st = dict(self.__dict__)
        st.pop("_packed", None)
        st.pop("_p2p_flat", None)
        st.pop("_locate", None)
        st.pop("_merge_stable", None)   # (a note of mldivide's to itself: see _passed_untouched)
        return st


class Polytope(object):
    """Convex polytope {x | A x <= b} (H-representation).

    Attributes `A`, `b`, `minrep`, `bbox`, `fulldim`, `vertices`, and the cached Chebyshev
    ball `chebR` / `chebXc` behave as in the reference (polytope/polytope.py:89-148).
    With `normalize=True` rows are scaled to unit norm and rows with norm <= 1e-10 dropped.
    """

    def __init__(self, A=np.array([]), b=np.array([]), minrep=False, chebR=0, chebX=None,
                 fulldim=None, volume=None, vertices=None, normalize=True):
        done = False
        if normalize and type(A) is np.ndarray and type(b) is np.ndarray and A.dtype == _F64 and b.dtype == _F64 \
                and A.ndim == 2 and A.size > 0:
            # the usual call -- float64 arrays, every row stays -- without the wrappers around the same ufuncs (np.sum,
            # .min, astype + a second product): the constructor runs thousands of times per Region operation
            norms = np.sqrt(np.add.reduce(A * A, 1))
            if np.minimum.reduce(norms) > 1e-10:
                scale = 1 / norms
                self.A = A * scale[:, None]
                self.b = b.ravel() * scale
                done = True
        if not done:
            self.A = A.astype(float)
            self.b = b.astype(float).ravel()        # (a fresh 1-D array: astype copied)
        if A.size > 0 and normalize and not done:
            norms = np.sqrt(np.sum(A * A, 1)).ravel()
            if norms.min() > 1e-10:
                # every row stays (the usual case): the same products without the index round trip -- a quarter of the
                # constructor's time, and a Region operation at C4 size builds ~5 000 polytopes
                scale = 1 / norms
                self.A = self.A * scale[:, None]
                self.b = self.b * scale
            else:
                rows = np.nonzero(norms > 1e-10)[0]
                scale = 1 / norms[rows]
                self.A = self.A[rows, :] * scale[:, None]   # row-wise multiply by the reciprocal norm
                self.b = self.b[rows].flatten() * scale
        self.minrep = minrep
        self._chebXc = chebX
        self._chebR = chebR
        self.bbox = None
        self.fulldim = fulldim
        self._volume = None
        if volume is not None:
            self._set_volume(volume)
        self.vertices = vertices

    def __str__(self):
        """The H-representation as the reference prints it (ref :150-176, pinned by its test_polytope_str): numpy's
        rendering of A and of b as a column, side by side, ' x <= ' on the middle row."""
        left = str(self.A).split("\n")
        right = str(self.b.reshape(-1, 1) if self.b.ndim == 1 else self.b).split("\n")
        n = len(left)
        at = (n - 1) // 2
        out = []
        for k in range(n):
            if k == at:
                mid = " x <= "
            elif k == n - 1:
                mid = "|    "
            else:
                mid = " |    "
            out.append(left[k] + mid + right[k])
        return "Single polytope \n  " + "\n  ".join(out) + "\n"

    def __len__(self):
        return 0

    def __copy__(self):
        twin = Polytope(self.A, self.b)   # (the constructor copies: astype, then the row scaling)
        twin._chebXc, twin._chebR = self._chebXc, self._chebR
        twin.minrep, twin.bbox, twin.fulldim = self.minrep, self.bbox, self.fulldim
        return twin

    def copy(self):
        return self.__copy__()

    def __contains__(self, point):
        """`point in self`, boundary included up to the module tolerance ABS_TOL (ref :191-204)."""
        if not isinstance(point, np.ndarray):
            point = np.array(point)
        return bool(self.contains(point.flatten()[:, np.newaxis], ABS_TOL)[0])

    def contains(self, points, abs_tol=ABS_TOL):
        """Boolean array: which column vectors of `points` satisfy A x - b < abs_tol row-wise
        (strict; abs_tol=0 excludes the boundary).  ref :206-218."""
        return _contains_many([self], points, abs_tol, region=True)

    def nearest(self, points):
        """(x[N, d], dist[N]): the closest point of this polytope to every column of `points` ([d, N]); module-level nearest."""
        return nearest(self, points)

    def distance(self, points):
        """dist[N]: the Euclidean distance of every column of `points` ([d, N]) to this polytope."""
        return distance(self, points)

    def __eq__(self, other):
        return self <= other and other <= self

    def __ne__(self, other):
        return not self == other

    def __le__(self, other):
        return is_subset(self, other)

    def __ge__(self, other):
        return is_subset(other, self)

    def __bool__(self):
        return bool(self.volume > 0)

    __nonzero__ = __bool__
    __hash__ = object.__hash__

    def union(self, other, check_convex=False):
        return union(self, other, check_convex)

    def diff(self, other):
        return mldivide(self, other)

    def intersect(self, other, abs_tol=ABS_TOL):
        """Intersection with a Polytope (-> Polytope) or a Region (-> Region).  ref :255-275."""
        if isinstance(other, Region):
            return other.intersect(self, abs_tol=abs_tol)
        if not isinstance(other, Polytope):
            raise Exception("Polytope intersection defined only with other Polytope. Got instead: "
                            + str(type(other)))
        if (not is_fulldim(self)) or (not is_fulldim(other)):
            return Polytope()
        if self.dim != other.dim:
            raise Exception("polytopes have different dimension")
        return reduce(Polytope(np.vstack([self.A, other.A]), np.hstack([self.b, other.b])), abs_tol=abs_tol)

    def translation(self, d):
        """Copy of self moved by the vector d (ref :277-286, :449-466): b += A d."""
        out = self.copy()
        out.b = out.b + out.A.dot(np.asarray(d, dtype=float).flatten())
        if out._chebXc is not None:
            out._chebXc = out._chebXc + np.asarray(d, dtype=float).flatten()
        out.bbox = None
        return out

    @classmethod
    def from_box(cls, intervals=[]):
        """Hyperrectangle from [[x0_min, x0_max], ...] (ref :311-354)."""
        if not isinstance(intervals, np.ndarray):
            try:
                intervals = np.array(intervals)
            except Exception:
                raise Exception("Polytope.from_box:intervals must be a numpy ndarray or "
                                "convertible as arg to numpy.array")
        if intervals.ndim != 2:
            raise Exception("Polytope.from_box: intervals must be 2 dimensional")
        if intervals.shape[1] != 2:
            raise Exception("Polytope.from_box: intervals must have 2 columns")
        if (intervals[:, 0] > intervals[:, 1]).any():
            raise Exception("Polytope.from_box: Invalid interval in from_box method.\n"
                            "First element of an interval must not be larger than the second.")
        n = intervals.shape[0]
        return cls(np.vstack([np.eye(n), -np.eye(n)]), np.hstack([intervals[:, 1], -intervals[:, 0]]), minrep=True)

    def project(self, dim, solver=None, abs_tol=ABS_TOL, verbose=0):
        """Projection onto the coordinates `dim` (1-based): see `projection` (ref :356-362)."""
        return projection(self, dim, solver, abs_tol, verbose)

    def scale(self, factor):
        self.b = factor * self.b

    @property
    def dim(self):
        try:
            return np.shape(self.A)[1]
        except Exception:
            return 0.0

    @property
    def volume(self):
        if self._volume is None:
            self._volume = volume(self)
        return self._volume

    def _set_volume(self, polytope_volume):
        if polytope_volume < 0.0:
            raise ValueError("`polytope_volume` must be >= 0, given:  {v}".format(v=polytope_volume))
        self._volume = float(polytope_volume)

    @property
    def chebR(self):
        cheby_ball(self)
        return self._chebR

    @property
    def chebXc(self):
        cheby_ball(self)
        return self._chebXc

    @property
    def cheby(self):
        return cheby_ball(self)

    @property
    def bounding_box(self):
        if self.bbox is None:
            self.bbox = bounding_box(self)
        return self.bbox


# ======================================================================================
class Region(_NoDeviceState):
    """Possibly non-convex set: a list of convex polytopes (ref :650-936)."""

    def __init__(self, list_poly=None, props=None):
        if list_poly is None:
            list_poly = []
        if props is None:
            props = set()
        if isinstance(list_poly, str):
            # the reference's hack for discrete problems (ref :681-685)
            self.list_poly = list_poly
            self.props = set(props)
            return
        if isinstance(list_poly, Region):
            dim = list_poly[0].dim
            for poly in list_poly:
                if poly.dim != dim:
                    raise Exception("Region error: Polytopes must be of same dimension!")
        empties = [p for p in list_poly if is_empty(p)]
        if not empties:
            self.list_poly = list(list_poly)
        else:
            # the reference takes every empty member out with list.remove (ref :694-696): the first element that IS it or
            # compares equal to it -- another empty one, or an earlier member whose sampled volume is below 1e-7 (`==` is
            # "both differences have a volume below 1e-7", ref :220-230)
            self.list_poly = list(list_poly)
            for poly in empties:
                for k, e in enumerate(self.list_poly):
                    if e is poly or is_empty(e):
                        del self.list_poly[k]
                        break
                    if e._chebR and e._chebXc is not None and \
                            _unit_ball_volume(e.A.shape[1]) * float(e._chebR) ** e.A.shape[1] >= 1e-6:
                        continue   # (a cached ball of that volume: its sampled volume is nowhere near 1e-7)
                    if e == poly:
                        del self.list_poly[k]
                        break
        self.props = set(props)
        self.bbox = None
        self.fulldim = None
        self._volume = None
        self._chebXc = None
        self._chebR = None

    def __iter__(self):
        return iter(self.list_poly)

    def __getitem__(self, key):
        return self.list_poly[key]

    def __str__(self):
        out = ""
        for i, p in enumerate(self.list_poly):
            out += "\t Polytope number %d:\n\t %s\n" % (i + 1, str(p).replace("\n", "\n\t\t"))
        return out + "\n"

    def __len__(self):
        return len(self.list_poly)

    def __contains__(self, point):
        if not isinstance(point, np.ndarray):
            point = np.array(point)
        return any(point in u for u in self.list_poly)

    def contains(self, points, abs_tol=ABS_TOL):
        """OR over the polytopes of Polytope.contains (ref :732-746)."""
        if not isinstance(points, np.ndarray):
            points = np.array(points)
        if points.shape[0] != self.dim:
            raise ValueError("points should be column vectors")
        return _contains_many(self.list_poly, points, abs_tol, region=True, owner=self)

    def nearest(self, points):
        """(x[N, d], dist[N], member int32[N]): the closest point of the union of the members to every column of `points`
        ([d, N]) and the member it lies in (lowest index on ties); module-level nearest."""
        return nearest(self, points)

    def distance(self, points):
        """dist[N]: the Euclidean distance of every column of `points` ([d, N]) to this region."""
        return distance(self, points)

    def locate(self, points, abs_tol=ABS_TOL):
        """For each column of `points` the index into `list_poly` of the FIRST member that contains it, or -1 (int32[N];
        no counterpart in the reference, whose users loop `x in poly`).  Members with an empty description contain
        nothing.  On 'hip' the packed rows and the culling grid stay on this Region between calls (batch.locate_batch)."""
        if not isinstance(points, np.ndarray):
            points = np.array(points)
        if points.shape[0] != self.dim:
            raise ValueError("points should be column vectors")
        return _locate_many(self.list_poly, points, abs_tol, owner=self, table_owner=self)

    def __eq__(self, other):
        return self <= other and other <= self

    def __ne__(self, other):
        return not self == other

    def __le__(self, other):
        return is_subset(self, other)

    def __ge__(self, other):
        return is_subset(other, self)

    __hash__ = object.__hash__

    def __add__(self, other):
        return union(self, other, check_convex=True)

    def __bool__(self):
        return bool(self.volume > 0)

    __nonzero__ = __bool__

    def union(self, other, check_convex=False):
        return union(self, other, check_convex)

    def __sub__(self, other):
        return mldivide(self, other)

    def diff(self, other):
        return mldivide(self, other)

    def __and__(self, other):
        return intersect(self, other)

    def intersect(self, other, abs_tol=ABS_TOL):
        """Pairwise intersections, kept when their Chebyshev radius exceeds abs_tol and merged
        with union(check_convex=True) in pair order (ref :815-830)."""
        if isinstance(other, Polytope):
            other = [other]
        pairs = [(p0, p1) for p0 in self for p1 in other]
        pieces = _intersect_pairs(pairs, abs_tol)
        if _use_hip():
            # the boxes union(check_convex) wants of every piece it is handed, in one batch instead of one per step
            todo = [q for q in pieces if q.A.size and q.bbox is None and q.cheby[0] > abs_tol]
            if len(todo) > 1 and len({q.A.shape[1] for q in todo}) == 1:
                for q, box in zip(todo, _bbox_raw(todo)):
                    q.bbox = box
        out = Region()
        for piece in pieces:
            rp, _ = piece.cheby
            if rp > abs_tol:
                out = union(out, piece, check_convex=True)
        return out

    def translation(self, d):
        return Region([p.translation(d) for p in self.list_poly], self.props.copy())

    def __copy__(self):
        return Region(list_poly=self.list_poly[:], props=self.props.copy())

    def copy(self):
        return self.__copy__()

    @property
    def dim(self):
        return np.shape(self.list_poly[0].A)[1]

    @property
    def volume(self):
        if self._volume is None:
            self._volume = volume(self)
        return self._volume

    def _set_volume(self, region_volume):
        if region_volume < 0.0:
            raise ValueError("`region_volume` must be >= 0, given:  {v}".format(v=region_volume))
        self._volume = float(region_volume)

    @property
    def chebR(self):
        cheby_ball(self)
        return self._chebR

    @property
    def chebXc(self):
        cheby_ball(self)
        return self._chebXc

    @property
    def cheby(self):
        return cheby_ball(self)

    @property
    def bounding_box(self):
        if self.bbox is None:
            self.bbox = bounding_box(self)
        return self.bbox


# ====================================================================================== helpers
def _pack(polys):
    """[Polytope] -> A[B, m_max, d], b[B, m_max], m[B] (rows zero-padded).  No per-polytope Python work beyond
    collecting the array references: one concatenate and one scatter."""
    B = len(polys)
    d = polys[0].A.shape[1]
    ms = np.fromiter((p.A.shape[0] for p in polys), dtype=np.int32, count=B)
    m_max = max(int(ms.max()), 1)
    if int(ms.min()) == m_max:   # same row count everywhere: the padded layout is the concatenation itself
        A = np.concatenate([p.A for p in polys]).reshape(B, m_max, d)
        b = np.concatenate([p.b for p in polys]).reshape(B, m_max)
        return np.ascontiguousarray(A, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64), ms
    A = np.zeros((B, m_max, d))
    b = np.zeros((B, m_max))
    total = int(ms.sum())
    if total:
        first = np.cumsum(ms) - ms
        owner = np.repeat(np.arange(B), ms)
        row = np.arange(total) - np.repeat(first, ms)
        A[owner, row] = np.concatenate([p.A for p in polys if p.A.shape[0]])
        b[owner, row] = np.concatenate([p.b for p in polys if p.A.shape[0]])
    return A, b, ms


def _torch_or_none():
    """torch when it can be imported (device tensors, torch's stream), else None: the library's host-pointer entry points
    take the numpy arrays as they are (the library copies them in and out itself)."""
    try:
        import torch
        return torch
    except Exception:  # pragma: no cover - torch is part of the image
        return None


class _PackedTable(object):
    """(A, b, m) of a list of polytopes packed once, and -- on the 'hip' backend with torch in the process -- resident on
    the device from the first call that needs it there: `dev()` returns the torch CUDA tensors the `*_batch` entry points
    take as they are (device pointers on torch's stream: nothing is packed or uploaded again).  Without torch `dev()` hands
    out the packed numpy arrays (host-pointer entry points).  polytope_amd.batch.h2d_bytes counts the upload.  Pickling /
    deep-copying a table keeps the host arrays only."""
    __slots__ = ("A", "b", "ms", "_dev")

    def __init__(self, packed):
        self.A, self.b, self.ms = packed
        self._dev = None

    def same_content(self, packed):
        A, b, ms = packed
        return A.shape == self.A.shape and np.array_equal(ms, self.ms) and np.array_equal(b, self.b) \
            and np.array_equal(A, self.A)

    def dev(self):
        if self._dev is None:
            torch = _torch_or_none()
            if torch is None:
                self._dev = (self.A, self.b, self.ms)
            else:
                from . import batch, _lib
                dev = torch.device("cuda", _lib.context().device)
                batch._count_h2d(self.A, self.b, self.ms)
                self._dev = tuple(torch.as_tensor(v).to(dev) for v in (self.A, self.b, self.ms))
        return self._dev

    def __getstate__(self):
        return (self.A, self.b, self.ms)

    def __setstate__(self, st):
        self.A, self.b, self.ms = st
        self._dev = None


_tables = {}          # key (identity of the members' arrays) -> _PackedTable, most recently used last
_TABLES_MAX = 8


def _table_of(polys, owner=None):
    """Packed table of a list of non-empty polytopes of one dimension.  Kept on `owner` (a Region: `_packed`) or in a small
    most-recently-used cache.  A remembered table is found by the identity of the members' A / b arrays and reused only
    if its CONTENT is still what the members hold now: the rows are packed on the host on every call (one concatenate,
    ~0.2 ms per 1000 members) and compared with the resident table's host copy, so arrays edited in place
    (`poly.b += margin`) get a new table -- `contains` in the reference reads A and b on every call (ref :217-218).
    What a hit saves is the upload and the device allocations."""
    key = tuple((id(p.A), id(p.b)) for p in polys)
    packed = _pack(polys)
    hit = getattr(owner, "_packed", None) if owner is not None else None
    tab = hit[1] if (hit is not None and hit[0] == key) else _tables.pop(key, None)
    if tab is not None and not tab.same_content(packed):
        tab = None
    if tab is None:
        tab = _PackedTable(packed)
    _tables.pop(key, None)
    while len(_tables) >= _TABLES_MAX:
        _tables.pop(next(iter(_tables)))
    _tables[key] = tab
    if owner is not None:
        try:
            owner._packed = (key, tab)
        except AttributeError:  # pragma: no cover
            pass
    return tab


def _contains_many(polys, points, abs_tol, region=True, owner=None):
    points = np.asarray(points, dtype=float)
    if _use_hip():
        solvers._require("hip")
        if points.ndim != 2:
            raise ValueError("points should be column vectors")
        polys = [p for p in polys if p.A.size > 0]  # an empty description contains nothing here
        if not polys or points.shape[1] == 0:
            return np.full(points.shape[1], False, dtype=bool)
        if polys[0].A.shape[1] > _MAX_DIM:
            raise ValueError("the 'hip' backend handles dimension <= %d, got %d" % (_MAX_DIM, polys[0].A.shape[1]))
        from .batch import contains_batch
        if owner is not None and len(polys) >= 8:
            # a Region asked again and again (volume(), point-in-region queries): its rows stay on the device
            At, bt, mt = _table_of(polys, owner).dev()
            pts = np.ascontiguousarray(points)
            from . import batch as _b
            _b._count_h2d(pts)
            if isinstance(At, np.ndarray):   # no torch in the process: host pointers all the way
                return contains_batch(At, bt, pts, abs_tol, m=mt, region=True).astype(bool)
            torch = _torch_or_none()
            Xt = torch.as_tensor(pts).to(At.device)
            return contains_batch(At, bt, Xt, abs_tol, m=mt, region=True).cpu().numpy().astype(bool)
        A, b, ms = _pack(polys)
        return contains_batch(A, b, np.ascontiguousarray(points), abs_tol, m=ms, region=True).astype(bool)
    # explicitly selected non-'hip' backend: the reference's own numpy expression (ref :217-218)
    inside = np.full(points.shape[1], False, dtype=bool)
    for p in polys:
        inside |= np.all(p.A.dot(points) - p.b[:, np.newaxis] < abs_tol, axis=0)
    return inside


def _locate_many(polys, points, abs_tol, owner=None, table_owner=None):
    """Index into `polys` of the first polytope containing each column of `points`, or -1 (int32[N]).  'hip': the packed
    table comes from _table_of (kept on `table_owner`), and the LocateGrid built for it is kept on `owner` beside the
    table and abs_tol it was built for -- _table_of hands out the same table object as long as the rows' content is
    unchanged, so a second call uploads the points only."""
    points = np.asarray(points, dtype=float)
    if points.ndim != 2:
        raise ValueError("points should be column vectors")
    N = points.shape[1]
    if _use_hip():
        solvers._require("hip")
        idx = np.array([k for k, p in enumerate(polys) if p.A.size > 0], dtype=np.int64)
        if idx.size == 0 or N == 0:
            return np.full(N, -1, dtype=np.int32)
        members = [polys[k] for k in idx]
        if members[0].A.shape[1] > _MAX_DIM:
            raise ValueError("the 'hip' backend handles dimension <= %d, got %d" % (_MAX_DIM, members[0].A.shape[1]))
        from . import batch
        tab = _table_of(members, table_owner)
        At, bt, mt = tab.dev()
        grid = None
        if len(members) >= batch._LOCATE_AUTO_P:
            hit = owner.__dict__.get("_locate") if owner is not None else None
            if hit is not None and hit[0] is tab and hit[1] == float(abs_tol):
                grid = hit[2]
            else:
                grid = batch.locate_grid(At, bt, mt, abs_tol)
                if owner is not None:
                    owner.__dict__["_locate"] = (tab, float(abs_tol), grid)
        pts = np.ascontiguousarray(points)
        if isinstance(At, np.ndarray):   # no torch in the process: host pointers all the way
            first = batch.locate_batch(At, bt, pts, abs_tol, m=mt, grid=grid)
        else:
            batch._count_h2d(pts)
            Xt = _torch_or_none().as_tensor(pts).to(At.device)
            first = batch.locate_batch(At, bt, Xt, abs_tol, m=mt, grid=grid).cpu().numpy()
        return np.where(first >= 0, idx[np.maximum(first, 0)], -1).astype(np.int32)
    # explicitly selected non-'hip' backend: the reference's own numpy expression (ref :217-218), last member first
    first = np.full(N, -1, dtype=np.int32)
    for k in range(len(polys) - 1, -1, -1):
        p = polys[k]
        if p.A.size == 0:
            continue
        first[np.all(p.A.dot(points) - p.b[:, np.newaxis] < abs_tol, axis=0)] = k
    return first


def _ball_from_lp(status, r, xc):
    """cheby_ball's reading of the LP result (ref :1289-1297): (r, xc) or None for 'empty'."""
    if status != 0 or r < 0:
        return None
    return np.double(r), np.array(xc)


def _cheby_raw(polys, failed=None):
    """Chebyshev LP (F1) of each non-empty polytope -> list of (r, xc) or None.
    `failed` (a list, optional) receives the positions whose LP ended with a status other than 0."""
    if not polys:
        return []
    d = polys[0].A.shape[1]
    if _use_hip() and all(_fits_lp(p.A.shape[0], p.A.shape[1]) and p.A.shape[1] == d for p in polys):
        from .batch import cheby_ball_batch
        out = [None] * len(polys)
        # stacks of more than 64 rows take the LDS-resident engine: keep them out of the batch of the small ones
        big = [k for k, p in enumerate(polys) if p.A.shape[0] > _MAX_ROWS]
        small = [k for k, p in enumerate(polys) if p.A.shape[0] <= _MAX_ROWS]
        for idx in (small, big):
            if not idx:
                continue
            A, b, ms = _pack([polys[k] for k in idx])
            res = cheby_ball_batch(A, b, m=ms)
            for t, k in enumerate(idx):
                out[k] = _ball_from_lp(int(res["status"][t]), float(res["r"][t]), res["xc"][t])
                if failed is not None and int(res["status"][t]) != 0:
                    failed.append(k)
        return out
    out = []
    for p in polys:
        n = p.A.shape[1]
        c = np.negative(np.r_[np.zeros(n), 1])
        G = np.c_[p.A, np.sqrt(np.sum(p.A * p.A, axis=1))]
        sol = lpsolve(c, G, p.b)
        out.append(_ball_from_lp(sol["status"], sol["x"][-1], sol["x"][0:-1]) if sol["status"] == 0 else None)
        if failed is not None and sol["status"] != 0:
            failed.append(len(out) - 1)
    return out


def _cheby_fill(polys):
    """Compute and cache the Chebyshev ball of every polytope of the list that lacks one."""
    todo = [p for p in polys
            if not (p._chebXc is not None and p._chebR is not None) and not is_empty(p)]
    for p, ball in zip(todo, _cheby_raw(todo)):
        if ball is not None:
            p._chebR, p._chebXc = ball


# ====================================================================================== predicates
def is_empty(polyreg):
    """True if the DESCRIPTION is empty (no rows / no non-empty member), ref :939-959."""
    n = len(polyreg)
    if n == 0:
        try:
            return len(polyreg.A) == 0
        except Exception:
            return True
    return all(is_empty(p) for p in polyreg.list_poly)


def cheby_ball(poly1):
    """Chebyshev radius and a centre of a Polytope; for a Region the largest ball of its
    members (first maximum wins).  Returns cached values when present (ref :1241-1300)."""
    if (poly1._chebXc is not None) and (poly1._chebR is not None):
        return poly1._chebR, poly1._chebXc
    if isinstance(poly1, Region):
        _cheby_fill(poly1.list_poly)
        maxr, maxx = 0, None
        for p in poly1.list_poly:
            rc, xc = cheby_ball(p)
            if rc > maxr:
                maxr, maxx = rc, xc
        poly1._chebXc, poly1._chebR = maxx, maxr
        return maxr, maxx
    if is_empty(poly1):
        return 0, None
    ball = _cheby_raw([poly1])[0]
    if ball is None:
        return 0, None
    poly1._chebR, poly1._chebXc = ball
    return poly1._chebR, poly1._chebXc


def is_fulldim(polyreg, abs_tol=ABS_TOL):
    """True if the polytope / some member of the region has interior points (ref :962-985)."""
    if polyreg.fulldim is not None:
        return polyreg.fulldim
    if len(polyreg) == 0:
        rc, _ = cheby_ball(polyreg)
        status = rc > abs_tol
    else:
        _cheby_fill(polyreg.list_poly)
        status = any(cheby_ball(p)[0] > abs_tol for p in polyreg.list_poly)
    polyreg.fulldim = status
    return status


def is_inside(polyreg, point, abs_tol=ABS_TOL):
    """Deprecated spelling of `point in polyreg` with an explicit tolerance (ref :1017-1029)."""
    warnings.warn("Write `point in polyreg` instead of calling this function.", DeprecationWarning)
    if not isinstance(point, np.ndarray):
        point = np.array(point)
    return polyreg.contains(point[:, np.newaxis], abs_tol)[0]


def is_subset(small, big, abs_tol=ABS_TOL):
    r"""small \subseteq big, decided by the volume of small \ big (ref :1032-1050)."""
    for x in [small, big]:
        if not isinstance(x, (Polytope, Region)):
            raise TypeError("Not a Polytope or Region, got instead:\n\t" + str(type(x)))
    if _use_hip() and _inside_by_boxes(small, big):
        return True
    return bool(small.diff(big).volume < abs_tol)


def _inside_by_boxes(small, big):
    r"""True when the bounding boxes ALREADY CACHED on the members of `small` show that small \ big is empty for a convex
    `big` (one member): row j of big can be exceeded on a member's box by at most  sum_k max(a_jk l_k, a_jk u_k) - b_j,
    and a piece  member /\ {a_j x >= b_j}  of region_diff (ref :2190-2282) holds no ball of radius above half of that --
    below 2 ABS_TOL every piece is dropped, the difference is empty and its volume 0.  Nothing is computed here but
    array arithmetic on what is cached (Partition.refines fills the boxes of all its elements in one batch first);
    False means "not shown", never "not a subset"."""
    bigs = _members(big)
    smalls = _members(small)
    if len(bigs) != 1 or not smalls or any(p.bbox is None for p in smalls):
        return False
    Q = bigs[0]
    if Q.A.shape[1] != smalls[0].A.shape[1]:
        return False
    lo = np.hstack([p.bbox[0] for p in smalls])     # d x k
    hi = np.hstack([p.bbox[1] for p in smalls])
    if not (np.all(np.isfinite(lo)) and np.all(np.isfinite(hi))):
        return False
    reach = np.maximum(Q.A[:, :, None] * lo[None, :, :], Q.A[:, :, None] * hi[None, :, :]).sum(axis=1)   # rows x k
    return bool(np.all(reach - Q.b[:, None] <= 2 * ABS_TOL - 1e-9))


# ====================================================================================== bounding box
def _bbox_packed(polys):
    """_bbox_raw for polytopes of one dimension on the 'hip' backend, with array operations only (no per-LP
    Python objects).  The fused kernel (Chebyshev LP + 2d LPs from its centre per polytope, one launch; for d > 8 the
    2d LPs without a stored dictionary, at most 64 rows); polytopes it hands back (empty, flat, unbounded ball) and
    longer d > 8 stacks go down as ONE batch of 2d generic LPs each.
    Same status handling as the reference (:1372-1409)."""
    from .batch import bbox_batch, lpsolve_batch
    d = polys[0].A.shape[1]
    ms = np.array([p.A.shape[0] for p in polys], dtype=np.int32)
    m_max = max(int(ms.max()), 1)
    B = len(polys)
    A3 = np.zeros((B, m_max, d))
    b3 = np.zeros((B, m_max))
    for k, p in enumerate(polys):
        A3[k, :ms[k]] = p.A
        b3[k, :ms[k]] = p.b
    lo = np.empty((B, d))
    hi = np.empty((B, d))
    rest = np.arange(B)
    if int(ms.min()) >= 1 and (d <= 8 or m_max <= 64):
        res = bbox_batch(A3, b3, m=ms)
        done = res["status"] == 0
        lo[done], hi[done] = res["lb"][done], res["ub"][done]
        rest = np.nonzero(~done)[0]
    if rest.size:
        nr = rest.size
        cost = np.vstack([np.eye(d), -np.eye(d)])                  # lower_0..lower_{d-1}, upper_0..upper_{d-1}
        res = lpsolve_batch(np.tile(cost, (nr, 1)), np.repeat(A3[rest], 2 * d, axis=0),
                            np.repeat(b3[rest], 2 * d, axis=0), m=np.repeat(ms[rest], 2 * d))
        st = res["status"].reshape(nr, 2, d)
        xi = res["x"].reshape(nr, 2, d, d)[:, :, np.arange(d), np.arange(d)]   # x[i] of LP i
        bad = ~np.isin(st, (0, 2, 3))
        if bad.any():
            k, side, i = np.argwhere(bad)[0]
            raise RuntimeError("bounding_box (%s corner): `polytope.solvers.lpsolve` returned:  {'status': %d, "
                               "'x': None, 'fun': None}\nits docstring describes return values"
                               % ("lower" if side == 0 else "upper", int(st[k, side, i])))
        lo[rest] = np.where(st[:, 0] == 0, xi[:, 0], np.where(st[:, 0] == 3, -np.inf, 0.0))
        hi[rest] = np.where(st[:, 1] == 0, xi[:, 1], np.where(st[:, 1] == 3, np.inf, lo[rest]))
    return [(lo[k].reshape(d, 1).copy(), hi[k].reshape(d, 1).copy()) for k in range(B)]


def _bbox_raw(polys):
    """Bounding boxes of non-empty Polytopes via 2d LPs each (F3), all in one batch."""
    if _use_hip() and polys and len({p.A.shape[1] for p in polys}) == 1 and all(
            p.A.ndim == 2 and _fits(p.A.shape[0], p.A.shape[1]) for p in polys):
        return _bbox_packed(polys)
    cs, Gs, hs = [], [], []
    for p in polys:
        n = p.A.shape[1]
        eye = np.eye(n)
        for i in range(n):
            cs.append(eye[:, i]); Gs.append(p.A); hs.append(p.b)
        for i in range(n):
            cs.append(-eye[:, i]); Gs.append(p.A); hs.append(p.b)
    if _use_hip() and len({c.size for c in cs}) > 1:
        sols = [solvers.lpsolve(c, G, h) for c, G, h in zip(cs, Gs, hs)]
    else:
        sols = solvers.lpsolve_many(cs, Gs, hs)
    out, pos = [], 0
    for p in polys:
        n = p.A.shape[1]
        lo, hi = np.zeros([n, 1]), np.zeros([n, 1])
        for i in range(n):
            sol = sols[pos + i]
            if sol["status"] == 0:
                lo[i] = sol["x"][i]
            elif sol["status"] == 3:
                lo[i] = -np.inf
            elif sol["status"] == 2:
                lo[i] = 0
            else:
                raise RuntimeError("bounding_box (lower corner): `polytope.solvers.lpsolve` returned:  "
                                   "{v}\nits docstring describes return values".format(v=sol))
        for i in range(n):
            sol = sols[pos + n + i]
            if sol["status"] == 0:
                hi[i] = sol["x"][i]
            elif sol["status"] == 3:
                hi[i] = np.inf
            elif sol["status"] == 2:
                hi[i] = lo[i]
            else:
                raise RuntimeError("bounding_box (upper corner): `polytope.solvers.lpsolve` returned:  "
                                   "{v}\nits docstring describes return values".format(v=sol))
        out.append((lo, hi))
        pos += 2 * n
    return out


def bounding_box(polyreg):
    """Smallest axis-aligned box (l, u), each a (d,1) array; cached in `.bbox` (ref :1314-1411)."""
    if polyreg.bbox is not None:
        return polyreg.bbox
    if isinstance(polyreg, Region):
        members = polyreg.list_poly
        if not members:
            polyreg.dim   # (a Region without members: the reference fails on `.dim` here, IndexError, ref :1330-1332)
        todo = [p for p in members if p.bbox is None]
        for p, box in zip(todo, _bbox_raw(todo)):
            p.bbox = box
        lows = np.array([p.bbox[0].ravel() for p in members])
        highs = np.array([p.bbox[1].ravel() for p in members])
        l = lows.min(axis=0).reshape(-1, 1)
        u = highs.max(axis=0).reshape(-1, 1)
        polyreg.bbox = l, u
        return l, u
    polyreg.bbox = _bbox_raw([polyreg])[0]
    return polyreg.bbox


def _bounding_box_to_polytope(lower, upper):
    return box2poly([(a[0], b[0]) for a, b in zip(lower, upper)])


def box2poly(box):
    """Polytope from [[x1min, x1max], [x2min, x2max], ...] (ref :2293-2299)."""
    return Polytope.from_box(box)


# ====================================================================================== reduce
def _reduce_lp_loop(poly, nonEmptyBounded, abs_tol):
    """reduce() with the LPs issued one by one through lpsolve (non-'hip' backends, and the
    little-used nonEmptyBounded=0 variant).  Steps as ref :1084-1163."""
    A_arr, b_arr = poly.A, poly.b
    rows = np.nonzero(poly.b != np.inf)
    A_arr, b_arr = A_arr[rows], b_arr[rows]
    neq = A_arr.shape[0]
    inv = 1 / np.sqrt(np.sum(A_arr.T ** 2, 0))
    unit = np.dot(A_arr.T, np.diag(inv)).T
    drop = set()
    for i in range(neq):
        for j in range(i + 1, neq):
            if np.dot(unit[i].T, unit[j]) > 1 - abs_tol:
                drop.add(j if b_arr[i] * inv[i] < b_arr[j] * inv[j] else i)
    keep = [i for i in range(neq) if i not in drop]
    A_arr, b_arr = A_arr[keep], b_arr[keep]
    neq, nx = A_arr.shape
    if nonEmptyBounded and neq <= nx + 1:
        return Polytope(A_arr, b_arr)
    if neq > 3 * nx:
        lb, ub = Polytope(A_arr, b_arr).bounding_box
        cand = ~(np.dot((A_arr > 0) * A_arr, ub - lb) - (np.array([b_arr]).T - np.dot(A_arr, lb)) < -1e-4)
        A_arr, b_arr = A_arr[cand.squeeze()], b_arr[cand.squeeze()]
    neq, nx = A_arr.shape
    if nonEmptyBounded and neq <= nx + 1:
        return Polytope(A_arr, b_arr)
    kept = []
    for k in range(neq):
        b_arr[k] += 0.1
        sol = lpsolve(-A_arr[k, :], A_arr, b_arr)
        b_arr[k] -= 0.1
        if sol["status"] == 0:
            if -sol["fun"] - b_arr[k] > abs_tol:
                kept.append(k)
        elif sol["status"] == 3:
            kept.append(k)
    out = Polytope(A_arr[kept], b_arr[kept])
    out.minrep = True
    return out


def _reduce_many(polys, abs_tol):
    """Fused reduce of Polytopes that are neither minrep nor known to be flat -> list of Polytope.

    Side effects as in the reference: the Chebyshev ball and `fulldim` of each INPUT polytope
    are cached (is_fulldim at ref :1081)."""
    from .batch import reduce_batch, keep_to_bool
    big = [k for k, p in enumerate(polys) if p.A.shape[0] > _MAX_ROWS]
    if big and len(big) < len(polys):
        # polytopes of more than 64 rows take the LDS-resident kernel, one per wavefront: a batch of their own
        out = [None] * len(polys)
        small = [k for k, p in enumerate(polys) if p.A.shape[0] <= _MAX_ROWS]
        for sel in (small, big):
            for k, q in zip(sel, _reduce_many([polys[k] for k in sel], abs_tol)):
                out[k] = q
        return out
    A, b, ms = _pack(polys)
    res = reduce_batch(A, b, m=ms, abs_tol=abs_tol)
    masks = keep_to_bool(res["keep"], A.shape[1])
    # The fused kernels run unverified.  A polytope they call empty because their Chebyshev LP ended UNBOUNDED (or at a limit)
    # is a half-space or a cone as a rule -- the reference's verdict too (ref :1289-1297) -- but on rows a hair apart the
    # engine's pivot tolerance can call a bounded ball unbounded (tests/golden/g23).  Those few get the verified stand-alone
    # ball (one batch), and where that one is full-dimensional the reference's own LP loop on the verified LPs.
    redo = {}
    opened = [k for k in range(len(polys)) if int(res["flags"][k]) & _RF_F1OPEN]
    if opened:
        from .batch import cheby_ball_batch
        sub = cheby_ball_batch(A[opened], b[opened], m=ms[opened])
        for j, k in enumerate(opened):
            rj = float(sub["r"][j])
            if int(sub["status"][j]) == 0 and rj > abs_tol:
                p = polys[k]
                p._chebR, p._chebXc, p.fulldim = np.double(rj), np.array(sub["xc"][j], dtype=float), True
                redo[k] = _reduce_lp_loop(p, 1, abs_tol)
    out = []
    for k, p in enumerate(polys):
        if k in redo:
            out.append(redo[k])
            continue
        fl = int(res["flags"][k])
        if fl & _RF_LPFAIL:
            raise RuntimeError("bounding_box: an LP of the box prefilter of `reduce` ended with status 1 or 4")
        r = float(res["r"][k])
        if not np.isnan(res["xc"][k]).any():
            if p._chebXc is None or p._chebR is None:
                p._chebR, p._chebXc = np.double(r), res["xc"][k].copy()
        if p.fulldim is None:
            p.fulldim = bool(r > abs_tol) if abs_tol == ABS_TOL else p.fulldim
        if fl & _RF_EMPTY:
            out.append(Polytope())
            continue
        rows = np.nonzero(masks[k, :ms[k]])[0]
        if fl & _RF_MINREP:
            bk = (p.b[rows] + 0.1) - 0.1   # the h[k] += 0.1; h[k] -= 0.1 round trip of ref :1149-1151
            q = Polytope(p.A[rows], bk)
            q.minrep = True
        else:
            q = Polytope(p.A[rows], p.b[rows])
        # q is the same set as p: the ball the kernel found for p is a Chebyshev ball of q too (what a
        # cheby_ball(q) call would cache, ref :1298-1299), so callers that go on to is_fulldim / cheby_ball
        # -- intersect, envelope, union -- need no second LP
        if not np.isnan(res["xc"][k]).any():
            q._chebR, q._chebXc = np.double(r), res["xc"][k].copy()
        out.append(q)
    return out


def reduce(poly, nonEmptyBounded=1, abs_tol=ABS_TOL):
    """Remove redundant inequalities from the H-representation, one LP per facet
    (ref :1053-1163).  A Region is reduced member-wise; members that end up flat are dropped."""
    if isinstance(poly, Region):
        members = poly.list_poly
        results = [None] * len(members)
        if _use_hip() and nonEmptyBounded:
            todo = [k for k, p in enumerate(members)
                    if not p.minrep and p.fulldim is not False and p.A.size > 0
                    and _fits_reduce(p.A.shape[0], p.A.shape[1]) and np.all(np.isfinite(p.b))]
            if todo and len({members[k].A.shape[1] for k in todo}) == 1:
                for k, q in zip(todo, _reduce_many([members[k] for k in todo], ABS_TOL)):
                    results[k] = q
        lst = []
        for k, p in enumerate(members):
            red = results[k] if results[k] is not None else reduce(p)
            if is_fulldim(red):
                lst.append(red)
        return Region(lst, poly.props) if lst else Polytope()
    if poly.minrep:
        return poly
    if _use_hip() and nonEmptyBounded and poly.A.size > 0 and _fits_reduce(poly.A.shape[0], poly.A.shape[1]) \
            and np.all(np.isfinite(poly.b)) and poly.fulldim is not False:
        return _reduce_many([poly], abs_tol)[0]
    if not is_fulldim(poly):
        return Polytope()
    return _reduce_lp_loop(poly, nonEmptyBounded, abs_tol)


def _intersect_pairs(pairs, abs_tol):
    """Polytope.intersect for a list of (Polytope, Polytope) pairs; the stacked polytopes of all
    full-dimensional pairs are reduced in one batch."""
    involved = []
    for p0, p1 in pairs:
        involved += [p0, p1]
    _cheby_fill([p for p in involved if p.fulldim is None])
    out = [None] * len(pairs)
    stacks, where = [], []
    flat = None
    if _use_hip() and len(pairs) >= 8 and all(isinstance(p1, Polytope) for _, p1 in pairs):
        # Many pairs (a Region against a polytope): the bounding boxes of everything involved in ONE batch, and a pair whose
        # boxes overlap by less than 2 abs_tol in some coordinate is not stacked at all -- its intersection holds no ball of
        # radius abs_tol, `reduce` would return the empty polytope for it (ref :1081-1082).
        uniq = {}
        for p in involved:
            uniq.setdefault(id(p), p)
        full = [p for p in uniq.values() if p.A.size and is_fulldim(p)]
        todo = [p for p in full if p.bbox is None]
        if todo and len({p.A.shape[1] for p in todo}) == 1:
            for p, box in zip(todo, _bbox_raw(todo)):
                p.bbox = box
        if full and all(p.bbox is not None for p in full) and len({p.A.shape[1] for p in full}) == 1:
            pos = {id(p): i for i, p in enumerate(full)}
            lo = np.hstack([p.bbox[0] for p in full])   # d x n
            hi = np.hstack([p.bbox[1] for p in full])
            i0 = np.array([pos.get(id(p0), -1) for p0, _ in pairs])
            i1 = np.array([pos.get(id(p1), -1) for _, p1 in pairs])
            both = (i0 >= 0) & (i1 >= 0)
            ext = np.minimum(hi[:, i0], hi[:, i1]) - np.maximum(lo[:, i0], lo[:, i1])
            flat = both & np.any(ext <= 2 * abs_tol - 1e-9, axis=0)
    for k, (p0, p1) in enumerate(pairs):
        if not isinstance(p1, Polytope):
            raise Exception("Polytope intersection defined only with other Polytope. Got instead: " + str(type(p1)))
        if (not is_fulldim(p0)) or (not is_fulldim(p1)):
            out[k] = Polytope()
            continue
        if p0.dim != p1.dim:
            raise Exception("polytopes have different dimension")
        if flat is not None and flat[k]:
            out[k] = Polytope()
            continue
        stacks.append(Polytope(np.vstack([p0.A, p1.A]), np.hstack([p0.b, p1.b])))
        where.append(k)
    if stacks:
        batchable = _use_hip() and all(_fits_reduce(s.A.shape[0], s.A.shape[1]) for s in stacks) \
            and len({s.A.shape[1] for s in stacks}) == 1
        reduced = _reduce_many(stacks, abs_tol) if batchable else [reduce(s, abs_tol=abs_tol) for s in stacks]
        for k, q in zip(where, reduced):
            out[k] = q
    _cheby_fill([q for q in out if q.A.size > 0])
    return out


def intersect(poly1, poly2, abs_tol=ABS_TOL):
    """Intersection of two polytopes or regions (ref :1508-1526)."""
    if isinstance(poly1, Region):
        return poly1.intersect(poly2, abs_tol=abs_tol)
    if isinstance(poly2, Region):
        return poly2.intersect(poly1, abs_tol=abs_tol)
    if not isinstance(poly1, Polytope):
        raise Exception("poly1 not Region nor Polytope.Got instead: " + str(type(poly1)))
    return poly1.intersect(poly2, abs_tol)


def _pair_cell_ok(p):
    """A cell the listed-pair kernels take: a Polytope of 1..32 finite rows in dimension <= 16."""
    return isinstance(p, Polytope) and not isinstance(p, Region) and p.A.ndim == 2 and 1 <= p.A.shape[0] <= _MAX_ROWS // 2 \
        and 1 <= p.A.shape[1] <= _MAX_DIM and bool(np.all(np.isfinite(p.b))) and bool(np.all(np.isfinite(p.A)))


def intersect_pairs(cells, pairs, abs_tol=ABS_TOL):
    """[cells[i].intersect(cells[j], abs_tol) for i, j in pairs] -- the same arrays, `minrep` and cached Chebyshev ball per
    result, the same exceptions, `Polytope()` for a pair with an operand that is not full-dimensional.

    On the 'hip' backend the listed pairs of cells inside the kernels' envelope (Polytopes of 1..32 finite rows, one
    dimension <= 16) are ONE batch.intersect_pairs call on the cells' packed table (uploaded once, kept by _table_of): the
    stacks are formed, reduced and compacted on the device and only the results' rows come back.  Pairs the fused reduce
    leaves open (RF_F1OPEN) and pairs with a cell outside the envelope go through the single call.  On any other backend it
    is the loop.  (The balls of a batch may differ from the single call's in the last bits where the Chebyshev LP has ties,
    DESIGN 7; rows, minrep and verdicts do not.)"""
    cells = list(cells)
    plist = [(int(i), int(j)) for i, j in pairs]

    def single(i, j):
        return cells[i].intersect(cells[j], abs_tol)

    used = sorted({k for ij in plist for k in ij})
    if not _use_hip() or not plist or any(k < 0 or k >= len(cells) for k in used) \
            or not all(isinstance(cells[k], Polytope) for k in used):
        return [single(i, j) for i, j in plist]   # (a negative index, a Region, anything else: the loop's own behaviour)
    solvers._require("hip")
    ok = [k for k in used if _pair_cell_ok(cells[k])]
    if len({cells[k].A.shape[1] for k in ok}) > 1 or len({cells[k].dim for k in used if cells[k].A.size}) > 1:
        return [single(i, j) for i, j in plist]   # (mixed dimensions: the loop raises at the pair the reference raises at)
    _cheby_fill([cells[k] for k in ok if cells[k].fulldim is None])
    slot = {k: s for s, k in enumerate(k for k in ok if is_fulldim(cells[k]))}
    out = [None] * len(plist)
    batch_at = [t for t, (i, j) in enumerate(plist) if i in slot and j in slot and i != j]
    if batch_at:
        from . import batch
        members = [cells[k] for k in slot]
        At, bt, mt = _table_of(members).dev()
        listed = np.array([(slot[plist[t][0]], slot[plist[t][1]]) for t in batch_at], dtype=np.int32)
        if not isinstance(At, np.ndarray):
            torch = _torch_or_none()
            listed = torch.as_tensor(listed).to(At.device)
        res = batch.intersect_pairs(At, bt, listed, m=mt, abs_tol=abs_tol, rows=True)
        res = {k: (v if isinstance(v, np.ndarray) else v.cpu().numpy()) for k, v in res.items()}
        for q, t in enumerate(batch_at):
            fl = int(res["flags"][q])
            if fl & (_RF_F1OPEN | batch.RF_BADPAIR) or int(res["m"][q]) < 0:
                continue   # (left to the single call below)
            if fl & _RF_LPFAIL:
                raise RuntimeError("bounding_box: an LP of the box prefilter of `reduce` ended with status 1 or 4")
            if fl & _RF_EMPTY:
                out[t] = Polytope()
                continue
            mo = int(res["m"][q])
            poly = Polytope(res["A"][q, :mo], res["b"][q, :mo], normalize=False)
            poly.minrep = bool(fl & _RF_MINREP)
            if not np.isnan(res["xc"][q]).any():
                poly._chebR, poly._chebXc = np.double(res["r"][q]), res["xc"][q].copy()
            out[t] = poly
    for t, (i, j) in enumerate(plist):
        if out[t] is None:
            out[t] = single(i, j)
    return out


# ====================================================================================== union / convexity
def _members(s):
    if len(s) == 0:
        return [] if is_empty(s) else [s]
    return [p for p in s.list_poly if not is_empty(p)]


# Region.intersect / mldivide call union(check_convex=True) once per new piece, and every call repeats
# the greedy merge over ALL pieces gathered so far (ref :815-830, :1214-1224): the same groups are tested
# for convexity again and again.  The verdict is a pure function of the members' (A, b), so it is kept.
_convex_memo = {}
_CONVEX_MEMO_MAX = 50000
_hull_memo = {}          # ordered group of members (content) -> the merged convex piece of union(check_convex=True)
_HULL_MEMO_MAX = 20000


def _content_key(p):
    return (p.A.shape, p.A.tobytes(), p.b.tobytes())  # exact content (recomputed: arrays may be edited in place)


def union(polyreg1, polyreg2, check_convex=False):
    """Union as a Region of non-overlapping polytopes; with check_convex the pieces are greedily
    merged whenever their union is convex (ref :1166-1238)."""
    if is_empty(polyreg1):
        return polyreg2
    if is_empty(polyreg2):
        return polyreg1
    if check_convex:
        common = None
        if _use_hip():
            # Two polytopes whose bounding boxes overlap by less than 2 abs_tol in some coordinate (touching cells, cells
            # apart) have no full-dimensional intersection -- a ball inside it has a diameter of at most that overlap --,
            # which is all the reference asks of `common` here (ref :1182-1190).  The boxes are wanted by the greedy merge
            # below anyway; with them first, the repeated union of Region.intersect / mldivide (one piece joins k
            # non-overlapping ones, k times) skips k stacked reduce LPs and four device round trips per step.
            mem1, mem2 = _members(polyreg1), _members(polyreg2)
            todo = [p for p in mem1 + mem2 if p.bbox is None]
            for p, box in zip(todo, _bbox_raw(todo)):
                p.bbox = box
            if mem1 and mem2 and all(p.bbox is not None for p in mem1 + mem2):
                L1 = np.hstack([p.bbox[0] for p in mem1]); U1 = np.hstack([p.bbox[1] for p in mem1])   # d x k1
                flat = True
                for q in mem2:
                    ext = np.minimum(U1, q.bbox[1]) - np.maximum(L1, q.bbox[0])
                    if not bool(np.all(np.any(ext <= 2 * ABS_TOL - 1e-9, axis=0))):
                        flat = False
                        break
                if flat:
                    common = Polytope()
        if common is None:
            common = intersect(polyreg1, polyreg2)
        if is_fulldim(common):
            parts = [common, polyreg2.diff(polyreg1), polyreg1.diff(polyreg2)]
        else:
            parts = [common, polyreg1, polyreg2]
    else:
        parts = [polyreg1, polyreg2]
    lst = []
    for s in parts:
        lst += _members(s)
    if not check_convex:
        return Region(lst)
    if len(lst) <= 1:
        return Region(lst)
    # Bounding boxes of all pieces in one batch.  A candidate whose box is separated from the box of every
    # member of the (convex) group by a clear gap cannot make a convex union with it -- the union would not
    # even be connected, and is_convex would find the gap in envelope \ union -- so the envelope /
    # region_diff test is skipped for it; the outcome of the greedy merge (ref :1214-1224) is unchanged.
    todo = [p for p in lst if p.bbox is None and not is_empty(p)]
    for p, box in zip(todo, _bbox_raw(todo)):
        p.bbox = box
    if STRICT_REFERENCE_QUIRKS:
        _cheby_fill(lst)   # (one batch; _ref_index below reads the cached balls)
    gap_tol = 1e-4

    def apart(p, q):
        (pl, pu), (ql, qu) = p.bbox, q.bbox
        return bool(np.any(pl - qu > gap_tol) or np.any(ql - pu > gap_tol))

    final = []
    last_outer = None
    while lst:
        group = [lst[0]]
        for cand in lst[1:]:
            if cand.bbox is not None and all(m.bbox is not None and apart(cand, m) for m in group):
                convex = False
            else:
                group.append(cand)
                key = frozenset(_content_key(m) for m in group)
                convex = _convex_memo.get(key)
                if convex is None and _use_hip() and _clearly_not_convex(group):
                    convex = False
                    if len(_convex_memo) >= _CONVEX_MEMO_MAX:
                        _convex_memo.clear()
                    _convex_memo[key] = convex
                if convex is None:
                    convex, outer = is_convex(Region(group))
                    if convex and outer is not None:
                        # the envelope is_convex built for exactly these members in this order: the merged piece below is
                        # reduce(envelope(Region(group))) of the same list (ref :1226-1230) -- not computed a second time
                        last_outer = (tuple(id(m) for m in group), outer)
                    if len(_convex_memo) >= _CONVEX_MEMO_MAX:
                        _convex_memo.clear()
                    _convex_memo[key] = convex
                group.pop()
            if convex:
                group.append(cand)
            else:
                # the reference appends the candidate and, when the union is not convex, takes it out again with
                # list.remove (ref :1222-1226) -- which removes the FIRST element that compares equal, and Polytope.__eq__
                # is "both differences have a volume below 1e-7" (ref :220-230, :1032-1050): among pieces that small (a
                # simplex of radius 3e-3 in R^4 has a volume of 1e-10) an EARLIER member goes and the candidate stays
                k = _ref_index(group, cand)
                if k is not None:
                    del group[k]
                    group.append(cand)
        for poly in group:   # ... and the same for the group's members in the list (ref :1227-1228)
            k = _ref_index(lst, poly)
            del lst[len(lst) if k is None else k]
        # The merged piece is a pure function of the group's members (envelope + reduce of their rows), and the repeated
        # union of Region.intersect / mldivide (ref :815-830, :1484-1496) meets the same groups at every step: kept like
        # the convexity verdicts above (Region(1000 cells).intersect(P): 656 envelopes and 844 reduce calls without).
        hkey = tuple(_content_key(m) for m in group)
        piece = _hull_memo.get(hkey)
        if piece is None:
            if last_outer is not None and last_outer[0] == tuple(id(m) for m in group):
                hull = reduce(last_outer[1])
            else:
                hull = reduce(envelope(Region(group)))
            piece = reduce(hull) if not is_empty(hull) else hull
            if len(_hull_memo) >= _HULL_MEMO_MAX:
                _hull_memo.clear()
            _hull_memo[hkey] = piece.copy() if not is_empty(piece) else piece   # (private: callers may edit what they get)
        elif not is_empty(piece):
            if piece.bbox is None and _use_hip():
                piece.bounding_box   # (kept with the remembered piece: the next union asks for it at once, every time)
            piece = piece.copy()
        if not is_empty(piece):
            final.append(piece)
    return Region(final)


def _unit_ball_volume(d):
    from math import gamma, pi
    return pi ** (d / 2.0) / gamma(d / 2.0 + 1.0)


def _surely_not_inside(e, x):
    r"""True when a ball of volume >= 1e-6 lies in e and outside x (so volume(e \\ x) is nowhere near the 1e-7 below which the
    reference calls e a subset of x, ref :1032-1050): the Chebyshev ball of e, CACHED, shrunk to the amount by which its
    centre violates a row of x.  Array arithmetic only; False means "not shown"."""
    if e._chebXc is None or not e._chebR or not x.A.size:
        return False
    viol = float(np.max(x.A @ np.asarray(e._chebXc, dtype=float).ravel() - x.b))
    rho = min(float(e._chebR), viol)
    return rho > 0.0 and _unit_ball_volume(x.A.shape[1]) * rho ** x.A.shape[1] >= 1e-6


def _ref_index(seq, x):
    r"""Position of the element list.remove(x) would take out of a list of the reference's polytopes: the first one that IS x
    or compares equal to it -- `e == x` there is  volume(e \\ x) < 1e-7 and volume(x \\ e) < 1e-7  (ref :220-230, :1032-1050), which
    holds between ANY two pieces whose own volumes are that small (a simplex of radius 3e-3 in R^4).  The comparison itself
    (two differences and their sampled volumes) runs only where it can come out True: not when a ball of volume 1e-6 lies in
    one and outside the other (_surely_not_inside on the cached Chebyshev balls -- neighbouring pieces of any size that
    matters).  None: x is not in the list (cannot happen here)."""
    for k, e in enumerate(seq):
        if e is x:
            return k
        if not STRICT_REFERENCE_QUIRKS:
            continue      # (by identity only: the element itself)
        if not e.A.size or not x.A.size or _surely_not_inside(e, x) or _surely_not_inside(x, e):
            continue
        if e == x:
            return k
    return None


def _clearly_not_convex(group):
    r"""A cheap witness that the union of `group` is not convex, from Chebyshev balls that are already cached: for the
    newest member and each other one, the balls B(c1, r1) and B(c2, r2) lie in the union, so a convex union -- and the
    envelope is_convex builds (ref :988-1014) in any case -- holds B(mid, (r1 + r2) / 2), mid = (c1 + c2) / 2.  A point
    mid + (r1 + r2) / 4 u that every member excludes by a clear margin then sits, with a ball of radius (r1 + r2) / 4
    around it, inside the envelope and outside the union: envelope \ union is full-dimensional and the reference's test
    answers False.  Only array arithmetic on cached values; False means "no witness", not "convex".
    (Region(1000 cells).intersect(P), first call of a process: most of its ~900 convexity tests are such rejections, each an
    envelope, two reductions, bounding boxes and a region_diff.)"""
    cand = group[-1]
    if cand._chebXc is None or not cand._chebR or cand.A.size == 0:
        return False
    d = cand.A.shape[1]
    dirs = np.vstack([np.eye(d), -np.eye(d)])                 # 2d x d
    margin = 10 * ABS_TOL
    for m in group[:-1]:
        if m._chebXc is None or not m._chebR or m.A.size == 0 or m.A.shape[1] != d:
            continue
        step = 0.25 * (float(cand._chebR) + float(m._chebR))
        if not step > margin:
            continue
        mid = 0.5 * (np.asarray(cand._chebXc, dtype=float).ravel() + np.asarray(m._chebXc, dtype=float).ravel())
        pts = mid[None, :] + step * dirs                      # 2d x d
        out = np.full(pts.shape[0], np.inf)
        for q in group:
            if q.A.size == 0 or q.A.shape[1] != d:
                return False
            out = np.minimum(out, np.max(pts @ q.A.T - q.b[None, :], axis=1))   # how far outside q (rows are unit)
        if np.any(out > margin):
            return True
    return False


def _union_all(pieces):
    """res = Polytope(); for p in pieces: res = union(res, p, False)  (region_diff's accumulation, ref :2229, :2276) in
    one pass: the loop re-lists every member at every step (quadratic: 19 of 50 ms at config 4 under the profiler)."""
    lst = []
    for p in pieces:
        if not is_empty(p):
            lst += _members(p)
    if not lst:
        return Polytope()
    if len(lst) == 1 and len(pieces) >= 1:
        # union(empty, p) returns p itself (:1176-1179); a single Region piece stays a Region
        only = [p for p in pieces if not is_empty(p)]
        if len(only) == 1:
            return only[0]
    return Region(lst)


def is_convex(reg, abs_tol=ABS_TOL):
    """(True, envelope) if the region is convex, else (False, None) (ref :988-1014)."""
    if len(reg) == 0:
        return True, None
    outer = envelope(reg)
    if is_empty(outer):
        return False, None
    Pl, Pu = reg.bounding_box
    Ol, Ou = outer.bounding_box
    if np.any(abs(Pl - Ol) > abs_tol) or np.any(abs(Pu - Ou) > abs_tol):
        return False, None
    if is_fulldim(outer.diff(reg)):
        return False, None
    return True, outer


def _envelope_crossed_packed(members, abs_tol):
    """The (member, facet) pairs of envelope() that some other member reaches beyond, with every test polytope
    [p2; -row ii of p1] packed straight into ONE batch -- the constructor's row normalisation (ref :130-138)
    applied to the packed rows -- instead of one Polytope object per test.  None when it does not apply."""
    if not members:
        return set()
    d = members[0].A.shape[1]
    if not all(p.A.ndim == 2 and p.A.shape[1] == d and _fits(p.A.shape[0] + 1, d) for p in members):
        return None
    owner = [(i, ii, j) for i, p1 in enumerate(members) for ii in range(p1.A.shape[0])
             for j in range(len(members)) if j != i]
    if not owner:
        return set()
    from .batch import cheby_ball_batch
    m_max = max(p.A.shape[0] for p in members) + 1
    A3 = np.zeros((len(owner), m_max, d))
    b3 = np.zeros((len(owner), m_max))
    lens = np.empty(len(owner), dtype=np.int32)
    for t, (i, ii, j) in enumerate(owner):
        p1, p2 = members[i], members[j]
        m2 = p2.A.shape[0]
        A3[t, :m2] = p2.A
        b3[t, :m2] = p2.b
        A3[t, m2] = -p1.A[ii, :]
        b3[t, m2] = -p1.b[ii]
        lens[t] = m2 + 1
    norms = np.sqrt(np.sum(A3 * A3, 2))
    used = np.arange(m_max)[None, :] < lens[:, None]
    if not np.all(norms[used] > 1e-10):
        return None  # a (near-)zero row: the constructor would drop it
    scale = np.where(used, 1 / np.where(used, norms, 1.0), 0.0)
    out = cheby_ball_batch(A3 * scale[:, :, None], b3 * scale, m=lens)
    hit = (out["status"] == 0) & (out["r"] >= 0) & (out["r"] > abs_tol)
    return {(owner[t][0], owner[t][1]) for t in np.nonzero(hit)[0]}


def envelope(reg, abs_tol=ABS_TOL):
    """Polytope of all 'outer' inequalities of a region: facet ii of member i is outer when no
    other member reaches beyond it (one Chebyshev LP per (facet, other member)); empty Polytope
    when the envelope is not full-dimensional (ref :1414-1464)."""
    members = reg.list_poly
    if not members:   # (the reference ends up in Polytope(None, None) here, ref :1460-1464 -> :126)
        raise AttributeError("'NoneType' object has no attribute 'astype'")
    crossed = _envelope_crossed_packed(members, abs_tol) if _use_hip() else None
    if crossed is None:
        crossed = set()
        tests, owner = [], []
        for i, p1 in enumerate(members):
            for ii in range(p1.A.shape[0]):
                for j, p2 in enumerate(members):
                    if i == j:
                        continue
                    tests.append(Polytope(np.vstack([p2.A, -p1.A[ii, :]]), np.hstack([p2.b, -p1.b[ii]])))
                    owner.append((i, ii))
        balls = _cheby_raw(tests) if tests else []
        for (i, ii), ball in zip(owner, balls):
            if ball is not None and ball[0] > abs_tol:
                crossed.add((i, ii))
    Ae, be = [], []
    for i, p1 in enumerate(members):
        rows = [ii for ii in range(p1.A.shape[0]) if (i, ii) not in crossed]
        Ae.append(p1.A[rows, :])
        be.append(p1.b[rows])
    ret = reduce(Polytope(np.vstack(Ae), np.hstack(be)), abs_tol=abs_tol)
    return ret if is_fulldim(ret) else Polytope()


def _envelope_batch_dim(reg, abs_tol):
    """The dimension of a region whose facet tests the batched kernel takes, else None: the region goes through the single
    call (another backend, abs_tol <= 0, no members, an empty member or one known to be flat, mixed dimensions, d > 8, a
    member of more than 63 rows)."""
    from .batch import ENV_MAX_DIM, ENV_MAX_ROWS
    if not (_use_hip() and abs_tol > 0 and isinstance(reg, Region) and reg.list_poly):
        return None
    d = None
    for p in reg.list_poly:
        if not isinstance(p, Polytope) or p.A.ndim != 2 or p.A.size == 0 or p.fulldim is False:
            return None
        m, dp = p.A.shape
        if d is None:
            d = dp
        if dp != d or not 1 <= d <= ENV_MAX_DIM or m > ENV_MAX_ROWS:
            return None
    return d


def _envelope_stacks(regs, ks, abs_tol, info):
    """The outer rows of the regions regs[k], k in ks (all of one dimension, all taken by the kernel), gathered in member
    order and row order -> {k: Polytope of the stacked rows}; a region with a list entry that is not ENV_OK, or a row that
    is not unit length, is left out (the single call's)."""
    from .batch import envelope_outer_batch, ENV_OK
    table, pos, mem_idx, lens = [], {}, [], []
    for k in ks:   # every member once, however many regions (or entries) list it
        for p in regs[k].list_poly:
            if id(p) not in pos:
                pos[id(p)] = len(table)
                table.append(p)
            mem_idx.append(pos[id(p)])
        lens.append(len(regs[k].list_poly))
    A, b, ms = _pack(table)
    m_max = A.shape[1]
    live = np.arange(m_max)[None, :] < ms[:, None]
    unit = np.all(~live | (np.abs(np.sqrt(np.sum(A * A, 2)) - 1.0) < 1e-9), axis=1)   # (normalize=False members)
    mem_idx = np.asarray(mem_idx, dtype=np.int32)
    reg_off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    res = envelope_outer_batch(A, b, ms, reg_off, mem_idx, abs_tol)
    owner = np.repeat(np.arange(len(ks)), lens)
    bad = np.bincount(owner, weights=(res["status"] != ENV_OK) | ~unit[mem_idx], minlength=len(ks)) > 0
    bits = ((res["outer"][:, None] >> np.arange(m_max, dtype=np.uint64)[None, :]) & np.uint64(1)).astype(bool)
    bits &= ~bad[owner][:, None]
    e, r = np.nonzero(bits)   # (row-major: entries in list order, rows in row order)
    Af, bf = A[mem_idx[e], r], b[mem_idx[e], r]
    cut = np.concatenate([[0], np.cumsum(np.bincount(owner[e], minlength=len(ks)))])
    if info is not None:
        info["nlp"] += int(res["nlp"].sum())
        info["tests"] += int(sum((n - 1) * int(ms[mem_idx[lo:lo + n]].sum()) for lo, n in zip(reg_off[:-1], lens)))
        info["routed"] += int(bad.sum())
    return {k: Polytope(Af[cut[q]:cut[q + 1]], bf[cut[q]:cut[q + 1]]) for q, k in enumerate(ks) if not bad[q]}


def envelope_batch(regs, abs_tol=ABS_TOL, _info=None):
    """[envelope(r, abs_tol) for r in regs] with the facet tests of all regions in ONE launch
    (batch.envelope_outer_batch: one (region, member) entry per wavefront), their stacks of outer rows through one fused
    reduce and full dimension from one batch of Chebyshev balls.  A member listed by several regions is packed once.
    Everything the kernel does not take goes through envelope() itself and returns or raises what it does: a region with
    a list entry that is ENV_OPEN (a test at the threshold, or one without a verdict) or ENV_UNSUPPORTED, d > 8, a member of
    more than 63 rows, mixed dimensions, an empty member or one known to be flat, abs_tol <= 0, a backend other than 'hip'.
    `_info` (test hook): a dict that receives nlp (LPs the kernel ran), tests (LPs of the reference's loops for the same
    regions) and routed (regions the kernel handed back)."""
    regs = list(regs)
    out = [None] * len(regs)
    info = dict(nlp=0, tests=0, routed=0)
    groups = {}
    for k, reg in enumerate(regs):
        d = _envelope_batch_dim(reg, abs_tol)
        if d is not None:
            groups.setdefault(d, []).append(k)
    stacks = {}
    for d, ks in groups.items():
        stacks.update(_envelope_stacks(regs, ks, abs_tol, info))
    for d in groups:   # one fused reduce per dimension (as reduce() routes a single stack)
        todo = [k for k in groups[d] if k in stacks and stacks[k].A.size > 0 and np.all(np.isfinite(stacks[k].b))
                and _fits_reduce(stacks[k].A.shape[0], d)]
        for k, q in zip(todo, _reduce_many([stacks[k] for k in todo], abs_tol) if todo else []):
            out[k] = q
    for k, stack in stacks.items():
        if out[k] is None:
            out[k] = reduce(stack, abs_tol=abs_tol)
    _cheby_fill([out[k] for k in stacks if out[k].A.size > 0 and out[k].fulldim is None])
    for k in stacks:
        if not is_fulldim(out[k]):
            out[k] = Polytope()
    for k, reg in enumerate(regs):
        if k not in stacks:
            out[k] = envelope(reg, abs_tol)
    if _info is not None:
        _info.update(info)
    return out


def is_convex_batch(regs, abs_tol=ABS_TOL):
    """[is_convex(r, abs_tol) for r in regs]: (True, envelope) or (False, None) per region, (True, None) for one without
    members.  The envelopes come from envelope_batch (at the module's ABS_TOL, as is_convex builds them), the bounding
    boxes of all members and all envelopes from one batch, and for the regions the boxes leave undecided the differences
    envelope minus region from one region_diff_batch and the balls of all their pieces from one batch.  Between the
    stages only the survivors go on.  What envelope_batch hands to envelope() goes through is_convex() here."""
    regs = list(regs)
    out = [None] * len(regs)
    live = []
    for k, reg in enumerate(regs):
        if len(reg) == 0:
            out[k] = (True, None)
        elif _envelope_batch_dim(reg, ABS_TOL) is None or not abs_tol > 0:
            out[k] = is_convex(reg, abs_tol)
        else:
            live.append(k)
    info = {}
    env = dict(zip(live, envelope_batch([regs[k] for k in live], _info=info))) if live else {}
    for k in live:
        if is_empty(env[k]):
            out[k] = (False, None)
    live = [k for k in live if out[k] is None]
    # ---- the boxes: every member and every envelope that has none yet, one batch per dimension
    need = {}
    for k in live:
        for p in list(regs[k].list_poly) + [env[k]]:
            if p.bbox is None:
                need.setdefault(p.A.shape[1], {}).setdefault(id(p), p)
    for d, todo in need.items():
        todo = list(todo.values())
        for p, box in zip(todo, _bbox_raw(todo)):
            p.bbox = box
    for k in live:
        Pl, Pu = regs[k].bounding_box
        Ol, Ou = env[k].bounding_box
        if np.any(abs(Pl - Ol) > abs_tol) or np.any(abs(Pu - Ou) > abs_tol):
            out[k] = (False, None)
    live = [k for k in live if out[k] is None]
    # ---- envelope minus region, all at once; full dimension of the pieces from one batch of balls
    if live:
        diffs = region_diff_batch([env[k] for k in live], [regs[k] for k in live])
        pieces = [p for D in diffs for p in (D.list_poly if isinstance(D, Region) else [D]) if p.fulldim is None]
        _cheby_fill(pieces)
        for k, D in zip(live, diffs):
            out[k] = (False, None) if is_fulldim(D) else (True, env[k])
    return out


# ====================================================================================== difference
def mldivide(a, b, save=False):
    r"""Set difference a \ b as a Region (ref :1470-1505)."""
    if isinstance(b, Polytope):
        b = Region([b])
    if isinstance(a, Region):
        out = Region()
        subs = b.list_poly
        # Which subtrahends touch which member of the minuend at all?  A subtrahend whose intersection with `poly` has
        # radius < ABS_TOL leaves `poly` -- and every piece cut from it later -- unchanged (region_diff returns its
        # minuend when nothing intersects, ref :2154-2158), so the chain below skips it.  On the 'hip' backend the
        # Chebyshev LPs of ALL (member, subtrahend) stacks are one launch over the resident rows of both regions
        # (plp_overlap_cross); shapes the pair kernels do not take are screened member by member (one batch each).
        live_all = [c for c in subs if c.A.size]
        mine = [p for p in a if not is_empty(p)]
        touch = None
        packed = None
        if _use_hip() and len(subs) > 1 and mine:
            touch = _cross_touch(mine, live_all, a, b)
            if touch is None and len(live_all) > 1 and len({c.A.shape for c in live_all}) == 1:
                packed = (np.stack([c.A for c in live_all]), np.stack([c.b for c in live_all]))
        if touch is not None:
            # the Chebyshev balls region_diff wants of the subtrahends it visits (ref :2160-2165): every subtrahend that
            # touches some member, in ONE batch here instead of a small batch per member there
            need = np.flatnonzero(np.asarray(touch, dtype=bool).any(axis=0))
            _cheby_fill([live_all[i] for i in need if live_all[i].fulldim is None])
        # ... and the radius of [member; its first touching subtrahend] -- the opening scan of the first region_diff of every
        # member's chain (its minuend is still the member itself) -- for ALL members in one batch instead of one launch each
        # (is_subset(200 cells, 1000 cells): 200 launches of one LP, half of the call)
        first_r = None
        if touch is not None and len(live_all) == len(subs) and len(mine) > 1:
            tb = np.asarray(touch, dtype=bool)
            has = tb.any(axis=1)
            firsts = tb.argmax(axis=1)
            pairs = [(p, live_all[int(j)]) for p, h, j in zip(mine, has, firsts) if h]
            if len(pairs) > 1 and len({(p.A.shape, c.A.shape) for p, c in pairs}) == 1 and \
                    _fits_lp(pairs[0][0].A.shape[0] + pairs[0][1].A.shape[0], pairs[0][0].A.shape[1]):
                A3 = np.concatenate([np.stack([p.A for p, _ in pairs]), np.stack([c.A for _, c in pairs])], axis=1)
                b3 = np.concatenate([np.stack([p.b for p, _ in pairs]), np.stack([c.b for _, c in pairs])], axis=1)
                norms = np.sqrt(np.sum(A3 * A3, 2))
                if np.all(norms > 1e-10):   # (the constructor's row normalisation, ref :130-138, as _radii_stacked applies it)
                    from .batch import cheby_ball_batch
                    scale = 1 / norms
                    res_ = cheby_ball_batch(A3 * scale[:, :, None], b3 * scale)
                    ok_ = (res_["status"] == 0) & (res_["r"] >= 0)
                    first_r = {id(p): (c, np.double(rr) if o else 0) for (p, c), rr, o in zip(pairs, res_["r"], ok_)}
        row = 0
        live_pos = None   # positions of the non-empty subtrahends in `subs` (empty ones always stay in the chain)
        for poly in a:
            touching = subs
            if _use_hip() and len(subs) > 1 and not is_empty(poly):
                if touch is not None:
                    keep = np.asarray(touch[row], dtype=bool)
                    row += 1
                else:
                    keep = np.asarray(_radii_stacked(poly, live_all, packed)) >= ABS_TOL
                # (index arithmetic instead of a Python pass over every subtrahend per member: 200 members x 1000 cells
                # were 15 ms of is_subset's 49)
                if len(live_all) == len(subs):
                    sel = keep
                else:
                    if live_pos is None:
                        live_pos = np.array([i for i, c in enumerate(subs) if c.A.size], dtype=np.intp)
                    sel = np.ones(len(subs), dtype=bool)
                    sel[live_pos] = keep
                touching = [subs[i] for i in np.flatnonzero(sel)]
                skipped_before = np.diff(np.concatenate([[-1], np.flatnonzero(sel), [len(subs)]])) - 1
            else:
                skipped_before = np.zeros(len(touching) + 1, dtype=int)
            rest = poly
            for k_sub, sub in enumerate(touching):
                rest = _passed_untouched(rest, int(skipped_before[k_sub]))
                if k_sub == 0 and first_r is not None and first_r.get(id(poly)) is not None and first_r[id(poly)][0] is sub:
                    # the opening scan of this region_diff (ref :2148-2152) was part of the one batch above (formed with the
                    # member's rows before the skipped subtrahends' copies moved them by an ulp: the radius is read against
                    # 1e-7 only)
                    rest = region_diff(rest, sub, save=save, _Rc=[first_r[id(poly)][1]])
                else:
                    rest = mldivide(rest, sub, save=save)
            rest = _passed_untouched(rest, int(skipped_before[len(touching)]))
            out = union(out, rest, check_convex=True)
        return out
    if isinstance(a, Polytope):
        return region_diff(a, b)
    raise Exception("a neither Region nor Polytope")


def _renormalised(p, ops):
    """p after the arithmetic the reference's chain applies to a piece it does not change, `ops` a string of
      P  a pass through the constructor's row scaling (ref :130-138) -- what a copy is there (ref :178-185), and what envelope and
         reduce end with (ref :1460, :1162);
      R  reduce's in-place round trip of every right-hand side, h[k] = (h[k] + 0.1) - 0.1 (ref :1149-1151).
    Rows of norm 1 +- 1e-16 move by an ulp in the first pass or two and then stay: the loop ends when a whole cycle of `ops`
    changes nothing."""
    A, b = p.A, p.b
    if not A.size:
        return p
    changed = False
    k = 0
    quiet = 0
    only_p = "R" not in ops    # (a pass that changes nothing is followed by passes that change nothing: one quiet pass ends it)
    while k < len(ops) and quiet < (1 if only_p else 3):
        if ops[k] == "P":
            norms = np.sqrt(np.add.reduce(A * A, 1))
            if not np.minimum.reduce(norms) > 1e-10:
                return p.copy()   # (a row the constructor would drop: not a piece of a difference; the plain copy)
            if np.all(norms == 1.0):      # scaling by exactly 1: nothing moves (box rows; most rows after a pass or two)
                quiet += 1
                k += 1
                continue
            scale = 1 / norms
            A2, b2 = A * scale[:, None], b * scale
        else:
            A2, b2 = A, (b + 0.1) - 0.1
        if np.array_equal(A2, A) and np.array_equal(b2, b):
            quiet += 1
        else:
            A, b, changed, quiet = A2, b2, True, 0
        k += 1
    if not changed:
        return p
    q = Polytope(A, b, normalize=False)
    q._chebXc, q._chebR = p._chebXc, p._chebR
    q.minrep, q.bbox, q.fulldim = p.minrep, p.bbox, p.fulldim
    return q


def _passed_untouched(rest, nskipped):
    """What `nskipped` subtrahends that do not touch the minuend leave of `rest` in the reference's chain (ref :1484-1487).  A
    Polytope comes back from each region_diff as a COPY (ref :2128, :2157): one pass through the constructor's scaling.  A Region is
    taken apart and put together again (ref :1480-1488): member i of n is copied, then stands in n - i unions, each of which
    rebuilds it as reduce(envelope(.)) -- constructor, reduce's round trip of the right-hand sides (not for d + 1 rows or fewer:
    ref :1136-1138 returns early, and the piece is reduced three times), constructor.  The arithmetic matters: an ulp in a
    right-hand side decides which of two coinciding rows a later dedupe keeps (ref :1104-1109), i.e. the ORDER of a merged piece's
    rows."""
    if nskipped <= 0 or not STRICT_REFERENCE_QUIRKS or is_empty(rest):
        return rest
    while isinstance(rest, Region) and nskipped > 0 and not getattr(rest, "_merge_stable", False):
        # pieces as region_diff cut them have not been through the greedy convex merge yet: a subtrahend that does not
        # touch them takes them apart and puts them together with union(check_convex) (ref :1480-1488) -- pieces whose union
        # is convex become one, and list.remove's equality (union, above) may take a tiny piece out or keep one twice, again
        # at every pass.  Passes are run for real until one leaves the pieces as they were; the rest repeat its arithmetic.
        P = Region()
        for m in rest.list_poly:
            P = union(P, _renormalised(m, "P"), check_convex=True)
        nskipped -= 1
        if isinstance(P, Region) and len(P.list_poly) == len(rest.list_poly) and all(
                x.A.shape == y.A.shape and np.allclose(x.A, y.A, rtol=0, atol=1e-12) and np.allclose(x.b, y.b, rtol=0, atol=1e-12)
                for x, y in zip(P.list_poly, rest.list_poly)):
            P._merge_stable = True
        rest = P
    if nskipped <= 0 or is_empty(rest):
        return rest
    if isinstance(rest, Region):
        n = len(rest.list_poly)
        new = []
        for i, m in enumerate(rest.list_poly):
            cyc = "PPPP" if m.A.shape[0] <= m.A.shape[1] + 1 else "PRP"
            new.append(_renormalised(m, ("P" + cyc * (n - i)) * nskipped))
        if all(x is m for x, m in zip(new, rest.list_poly)):
            return rest
        out = Region(new, rest.props)
        out._merge_stable = True
        return out
    return _renormalised(rest, "P" * nskipped)


def _cross_touch(firsts, seconds, owner1=None, owner2=None):
    """bool[len(firsts), len(seconds)]: does the stack [first; second] have a Chebyshev radius >= ABS_TOL -- the opening scan
    of region_diff (ref :2148-2158) for every pair, one launch over the two lists' resident rows; None when the pair
    kernels do not take the shapes (more than 32 rows in a member, differing dimensions, too many pairs for one matrix)."""
    if not firsts or not seconds:
        return np.zeros((len(firsts), len(seconds)), dtype=bool)
    d = firsts[0].A.shape[1]
    if not (1 <= d <= _MAX_DIM) or any(p.A.shape[1] != d or not 1 <= p.A.shape[0] <= 32 for p in firsts + seconds):
        return None
    if len(firsts) * len(seconds) > (1 << 28):
        return None
    from .batch import overlap_cross
    A1, b1, m1 = _table_of(firsts, owner1).dev()
    A2, b2, m2 = _table_of(seconds, owner2).dev()
    mm = max(A1.shape[1], A2.shape[1])
    thresh = float(np.nextafter(ABS_TOL, 0.0))   # r > pred(ABS_TOL)  <=>  r >= ABS_TOL
    if isinstance(A1, np.ndarray):   # no torch in the process: the packed host arrays, host-pointer entry point
        def widen_np(A, b):
            if A.shape[1] == mm:
                return A, b
            return np.pad(A, ((0, 0), (0, mm - A.shape[1]), (0, 0))), np.pad(b, ((0, 0), (0, mm - b.shape[1])))
        A1, b1 = widen_np(A1, b1)
        A2, b2 = widen_np(A2, b2)
        got = overlap_cross(np.concatenate([A1, A2]), np.concatenate([b1, b2]), len(firsts),
                            m=np.concatenate([m1, m2]), thresh=thresh)
        return np.asarray(got).astype(bool)
    torch = _torch_or_none()

    def widen(A, b):
        if A.shape[1] == mm:
            return A, b
        return (torch.nn.functional.pad(A, (0, 0, 0, mm - A.shape[1])), torch.nn.functional.pad(b, (0, mm - b.shape[1])))
    A1, b1 = widen(A1, b1)
    A2, b2 = widen(A2, b2)
    got = overlap_cross(torch.cat([A1, A2]), torch.cat([b1, b2]), len(firsts), m=torch.cat([m1, m2]), thresh=thresh)
    return got.cpu().numpy().astype(bool)


def _radii_stacked(poly, others, packed=None):
    """Chebyshev radius (0 when the ball LP fails) of the stack [poly; c] for every c of `others`, as
    region_diff's own scan computes it (ref :2148-2152) -- including the constructor's row normalisation
    (ref :130-138) -- but packed straight into one batch instead of one Polytope object per stack.
    `packed`: (A[n, m, d], b[n, m]) of `others` when the caller has stacked them already (same shapes)."""
    if not others:
        return []
    same = _use_hip() and (packed is not None or len({c.A.shape for c in others}) == 1) and \
        _fits_lp(poly.A.shape[0] + others[0].A.shape[0], poly.A.shape[1])
    if same:
        n = len(others)
        oA, ob = packed if packed is not None else (np.stack([c.A for c in others]), np.stack([c.b for c in others]))
        A3 = np.concatenate([np.broadcast_to(poly.A, (n,) + poly.A.shape), oA], axis=1)
        b3 = np.concatenate([np.broadcast_to(poly.b, (n,) + poly.b.shape), ob], axis=1)
        norms = np.sqrt(np.sum(A3 * A3, 2))
        if np.all(norms > 1e-10):
            from .batch import cheby_ball_batch
            scale = 1 / norms
            out = cheby_ball_batch(A3 * scale[:, :, None], b3 * scale)
            ok = (out["status"] == 0) & (out["r"] >= 0)
            return [np.double(rr) if o else 0 for rr, o in zip(out["r"], ok)]
    return _radii([Polytope(np.vstack([poly.A, c.A]), np.hstack([poly.b, c.b])) for c in others])


def _radii(polys, nan_without_verdict=False):
    """Chebyshev radius of freshly built polytopes (0 when the ball LP fails), one batch.
    `nan_without_verdict`: NaN instead of 0 where the LP ended with a status other than 0."""
    out = []
    failed = [] if nan_without_verdict else None
    for k, (p, ball) in enumerate(zip(polys, _cheby_raw(polys, failed))):
        if ball is None:
            out.append(float("nan") if failed and k in failed else 0)
        else:
            p._chebR, p._chebXc = ball
            out.append(ball[0])
    return out


def _reduce_leaves(todo):
    """reduce() of the leaves of region_diff searches that the reference reduces (ref :2276), in order: one fused reduce
    launch for all that fit, reduce() itself for the rest."""
    done = [None] * len(todo)
    small = [k for k, p in enumerate(todo) if p.A.size > 0 and _fits_reduce(p.A.shape[0], p.A.shape[1])]
    if small:
        for k, q in zip(small, _reduce_many([todo[k] for k in small], ABS_TOL)):
            done[k] = q
    return [q if q is not None else reduce(p) for p, q in zip(todo, done)]


def region_diff(poly, reg, abs_tol=ABS_TOL, intersect_tol=ABS_TOL, save=False, _order=None, _Rc=None):
    """poly minus the union of the polytopes of reg, as non-overlapping pieces.

    The cells of `reg` are visited in the order argsort(-Rc) of the Chebyshev radii of their stacks with `poly`
    (ref :2153-2157).  Cells whose radii are mathematically equal -- on a grid every cell whose ball is limited by
    its own facets -- are ordered by the last-bit rounding of whichever LP code computed Rc, and the decomposition
    (a valid one either way) depends on that order.  `_order` (a permutation of range(len(reg)), test hook) replaces
    the argsort, so that the search can be compared with the reference's on such inputs (tests/golden g12 c4_order).

    Depth-first enumeration of the sign patterns of the subtrahends' new constraints, one
    Chebyshev LP per node (the algorithm of ref :2117-2282, same visiting order and the same
    tests).  The N LPs of the initial scan and the LPs of every level scan are independent and
    are issued as one batch each.
    """
    if not isinstance(poly, Polytope):
        raise Exception("poly not a Polytope, but: " + str(type(poly)))
    poly = poly.copy()
    if isinstance(reg, Polytope):
        reg = Region([reg])
    if not isinstance(reg, Region):
        raise Exception("reg not a Region, but: " + str(type(reg)))
    N = len(reg)
    if N == 0:
        reg = Region([reg])
        N = 1
    if is_empty(reg):
        return poly
    if is_empty(poly):
        return Polytope()
    cells = reg.list_poly
    # which cells meet the polytope at all
    # (`_Rc`: the caller has these radii already -- mldivide's one batch over all members of a Region)
    Rc = np.array(_radii_stacked(poly, cells) if _Rc is None or len(_Rc) != len(cells) else _Rc, dtype=float)
    N = int(np.sum(Rc >= intersect_tol))
    if N == 0:
        logger.debug("no Polytope in the Region intersects the given Polytope")
        return poly
    order = np.argsort(-Rc) if _order is None else np.asarray(_order, dtype=int)
    m = poly.A.shape[0]
    A = poly.A.copy()
    B = poly.b.copy()
    base = np.hstack([poly.A, poly.b[:, None]])
    _cheby_fill([cells[order[ii]] for ii in range(N) if cells[order[ii]].fulldim is None])
    mi = np.zeros(N, dtype=int)
    # constraints of the cells that are not already rows of poly (ref :2166-2183), all cells at once
    picked = [cells[order[ii]] for ii in range(N)]
    full = np.array([bool(is_fulldim(c)) for c in picked])
    if full.any():
        rows_all = np.vstack([np.hstack([c.A, c.b[:, None]]) for c, f in zip(picked, full) if f])
        owner = np.concatenate([np.full(c.A.shape[0], ii) for ii, (c, f) in enumerate(zip(picked, full)) if f])
        new = np.all(np.sum(np.abs(rows_all[:, None, :] - base[None, :, :]), axis=2) >= abs_tol, axis=1)
        mi = np.bincount(owner[new], minlength=N).astype(int)
        A = np.vstack([A, rows_all[new, :-1]])
        B = np.hstack([B, rows_all[new, -1]])
    if np.any(mi == 0):
        return Polytope()  # some cell covers the polytope
    M = int(np.sum(mi))
    beg = m + np.concatenate([[0], np.cumsum(mi[:-1])]).astype(int)
    A = np.vstack([A, -A[m:m + M, :]])
    B = np.hstack([B, -B[m:m + M]])
    res = Polytope()

    def poly_of(rows):
        if packed:
            # the constructor's row scaling (ref :130-138) acts row by row: An / Bn hold it for every row of the table
            # already (same ufuncs, same bits), so a piece is a gather -- 234 pieces at config 4: 3 ms -> 1 ms
            return Polytope(An[rows, :], Bn[rows], normalize=False)
        return Polytope(A[rows, :], B[rows])

    # All LPs of the search are Chebyshev LPs on row subsets of (A, B).  On the 'hip' backend they are
    # packed straight from the row lists -- after the constructor's normalisation (ref :130-138), which
    # acts row by row and is therefore applied once to all rows -- instead of going through one Polytope
    # object per candidate.
    norms = np.sqrt(np.sum(A * A, 1)).flatten()
    packed = _use_hip() and _fits(1, A.shape[1]) and bool(np.all(norms > 1e-10))
    if packed:
        from .batch import cheby_ball_batch
        scale = 1 / norms
        An, Bn = A * scale[:, None], B * scale
    if packed and abs_tol > 0 and not save and _RDIFF_NATIVE:
        # The search itself runs in the library (plp_region_diff_search; csrc/plp_rdiff_search.hpp): the reference's
        # visiting order and tests, LPs gathered on the device from the resident table by row index, one launch and
        # one synchronisation per visited node.  What comes back are the pieces as row lists, in order.
        from .batch import region_diff_search
        from ._lib import UnsupportedSize
        try:
            leaves, _stats = region_diff_search(An, Bn, m, mi, abs_tol)
        except UnsupportedSize:
            leaves = None   # a stack beyond what the library's search stages: the host twin below takes the call
        except ValueError as e:
            if "out of range" in str(e):
                raise IndexError("index out of bounds in region_diff (the reference's INDICES arithmetic, ref :2233)")
            raise
    else:
        leaves = None
    if leaves is not None:
        red = iter(_reduce_leaves([poly_of(rows) for kind, rows in leaves if kind == 1]))
        return _union_all([next(red) if kind == 1 else poly_of(rows) for kind, rows in leaves])

    def radii_rows(row_lists):
        """Chebyshev radius of the polytope of each row list, one batch: 0 for a ball LP solved with r < 0, NaN for one
        that ended without a verdict (any status but 0: the reference reads radius 0 there, ref :1294-1297, and
        solves again at every node below -- `_DiffSearch` must not take such a cell for empty for good)."""
        lens = [len(r) for r in row_lists]
        if not packed or max(lens) > _max_rows_lp(A.shape[1]):
            return _radii([poly_of(r) for r in row_lists], nan_without_verdict=True)
        res = [0] * len(row_lists)
        # stacks of more than 64 rows go to the LDS-resident engine in a batch of their own
        for sel in ([k for k, n_ in enumerate(lens) if n_ <= _MAX_ROWS], [k for k, n_ in enumerate(lens) if n_ > _MAX_ROWS]):
            if not sel:
                continue
            m_max = max(lens[k] for k in sel)
            A3 = np.zeros((len(sel), m_max, A.shape[1]))
            b3 = np.zeros((len(sel), m_max))
            for t, k in enumerate(sel):
                A3[t, :lens[k]] = An[row_lists[k]]
                b3[t, :lens[k]] = Bn[row_lists[k]]
            out = cheby_ball_batch(A3, b3, m=np.asarray([lens[k] for k in sel], dtype=np.int32))
            ok = (out["status"] == 0) & (out["r"] >= 0)
            for t, k in enumerate(sel):
                res[k] = np.double(out["r"][t]) if ok[t] else (0 if out["status"][t] == 0 else float("nan"))
        return res

    # Host twin of the library's search (csrc/plp_rdiff_search.hpp, plp_region_diff_search): the same state, moves and
    # inheritance of empty cells, driven through `radii_rows` -- what the non-'hip' backends run, and the A/B partner
    # of the library search on the GPU (tests: both must return the same pieces).
    search = _DiffSearch(m, mi, beg, M, abs_tol, radii_rows, look_ahead=packed)
    pieces = []
    for kind, rows in search.run():
        piece = poly_of(rows)
        pieces.append(reduce(piece) if kind == 1 else piece)
    return _union_all(pieces)


def region_diff_batch(polys, regs, abs_tol=ABS_TOL, intersect_tol=ABS_TOL, _info=None):
    """[region_diff(polys[k], regs[k], abs_tol, intersect_tol) for every k] with all searches in ONE launch.

    `regs`: one Region (or Polytope) shared by all polytopes, or one per polytope.  On the 'hip' backend the Chebyshev radii
    of all (polytope, cell) stacks come from one batch, the searches run one per wavefront (batch.region_diff_search_batch),
    and the pieces the reference reduce()s go through one fused reduce; the early exits of region_diff (empty region,
    empty polytope, nothing intersects, a cell that covers the polytope) are taken as there.  A problem beyond the kernel's
    caps (d > 4, more than 64 rows or cells, a list of more than 64 rows, the LP budget), or one on which the reference's
    index arithmetic raises IndexError, goes through region_diff itself.  On any other backend this is the loop.
    `_info` (test hook): a dict that receives Rc (per problem, the radii region_diff would compute; None where the
    problem never reached the batch), status and nlp."""
    from .batch import _rdiff_prepare, _rdiff_gather, region_diff_search_batch, RD_OK, RD_COVERED, RD_MAX_CELLS
    polys = list(polys)
    n = len(polys)
    regs = [regs] * n if isinstance(regs, (Polytope, Region)) else list(regs)
    if len(regs) != n:
        raise ValueError("region_diff_batch: one Region for all polytopes, or one per polytope")
    out = [None] * n
    info = dict(Rc=[None] * n, status=[None] * n, nlp=[None] * n)
    groups = {}   # dimension -> the problems that go into its launch
    for k in range(n):
        poly, reg = polys[k], regs[k]
        if isinstance(reg, Polytope):
            reg = Region([reg])
        batched = _use_hip() and _RDIFF_NATIVE and abs_tol > 0 and isinstance(poly, Polytope) and isinstance(reg, Region) \
            and len(reg) > 0 and not is_empty(reg) and not is_empty(poly)
        if batched:
            d = poly.A.shape[1]
            batched = _fits(poly.A.shape[0], d) and d <= 4 and len(reg) <= RD_MAX_CELLS and \
                all(c.A.ndim == 2 and c.A.shape[1] == d and 0 < c.A.shape[0] <= _MAX_ROWS for c in reg.list_poly)
        if not batched:
            out[k] = region_diff(polys[k], regs[k], abs_tol, intersect_tol)
            continue
        groups.setdefault(d, []).append((k, poly.copy(), reg))
    for d, members in groups.items():
        # the cell table: every Region once, its cells in order
        first, cells = {}, []
        for _, _, reg in members:
            if id(reg) not in first:
                first[id(reg)] = len(cells)
                cells.extend(reg.list_poly)
        B, m_max, mc_max = len(members), max(p.A.shape[0] for _, p, _ in members), max(c.A.shape[0] for c in cells)
        A, b, m = np.zeros((B, m_max, d)), np.zeros((B, m_max)), np.zeros(B, np.int32)
        CA, Cb, mc = np.zeros((len(cells), mc_max, d)), np.zeros((len(cells), mc_max)), np.zeros(len(cells), np.int32)
        for q, (_, p, _) in enumerate(members):
            m[q] = p.A.shape[0]
            A[q, :m[q]], b[q, :m[q]] = p.A, p.b
        for q, c in enumerate(cells):
            mc[q] = c.A.shape[0]
            CA[q, :mc[q]], Cb[q, :mc[q]] = c.A, c.b
        cell_off = np.concatenate([[0], np.cumsum([len(reg) for _, _, reg in members])]).astype(np.int64)
        cell_idx = np.concatenate([first[id(reg)] + np.arange(len(reg)) for _, _, reg in members]).astype(np.int64)
        pre = _rdiff_prepare(A, b, m, CA, Cb, mc, cell_off, cell_idx, intersect_tol, None)
        res = region_diff_search_batch(pre["A"], pre["b"], pre["m"], pre["CA"], pre["Cb"], pre["mc"], pre["cell_off"],
                                       pre["cell_idx"], abs_tol)
        _cheby_fill([cells[c] for c in sorted(set(int(c) for c in pre["cell_idx"])) if cells[c].fulldim is None])
        statuses, gathered = _rdiff_gather(pre, res)
        leaves, todo = {}, []
        for q, (k, p, reg) in enumerate(members):
            Rc = np.array(pre["Rc"][cell_off[q]:cell_off[q + 1]], dtype=float)
            status = int(statuses[q])
            info["Rc"][k], info["status"][k], info["nlp"][k] = Rc, status, int(res["nlp"][q])
            picked = pre["cell_idx"][pre["cell_off"][q]:pre["cell_off"][q + 1]]
            if len(picked) == 0:
                logger.debug("no Polytope in the Region intersects the given Polytope")
                out[k] = p
            elif status == RD_COVERED or not all(bool(is_fulldim(cells[c])) for c in picked):
                out[k] = Polytope()   # some cell covers the polytope
            elif status == RD_OK:
                leaves[q] = []
                for kind, Ak, bk in gathered[q]:
                    piece = Polytope(Ak, bk, normalize=False)
                    leaves[q].append((kind, piece))
                    if kind == 1:   # leaves the reference reduces (:2276)
                        todo.append(piece)
            else:   # beyond the kernel (or IndexError in the reference): the single call, with the radii it would compute
                out[k] = region_diff(polys[k], regs[k], abs_tol, intersect_tol, _Rc=Rc)
        red = iter(_reduce_leaves(todo))   # (one launch for the leaves of all problems)
        for q, (k, _, _) in enumerate(members):   # (in the order the leaves were queued)
            if q in leaves:
                out[k] = _union_all([next(red) if kind == 1 else piece for kind, piece in leaves[q]])
    if _info is not None:
        _info.update(info)
    return out


class _DiffSearch:
    """The search of region_diff (ref :2201-2281) over row lists of one constraint table: m rows of the minuend, then
    M = sum(mi) new rows of the cells (cell j from beg[j]), then their M negations.

    State: `counter[j]` (0 = cell j closed; c = its first c - 1 new rows kept, row c negated), `rows` (the reference's
    INDICES, Python's negative indices included) and `level`.  Moves: `scan` (first cell from `level` on whose stack
    with the current rows is full-dimensional), `next_sibling`, `reopen_after_piece`.  `run()` yields the pieces as
    (kind, rows): kind 0 = as is, 1 = to be reduce()d.  A cell whose stack had radius <= abs_tol / 2 at a scan is not
    solved again while the current rows contain that scan's rows (the set only shrinks below it)."""

    def __init__(self, m, mi, beg, M, abs_tol, radii_rows, look_ahead):
        self.m, self.mi, self.beg, self.M, self.tol = int(m), [int(v) for v in mi], [int(v) for v in beg], int(M), abs_tol
        self.N = len(self.mi)
        self.radii_rows = radii_rows
        self.look_ahead = look_ahead      # batched backends: solve the chain of siblings with the node
        self.counter = [0] * self.N       # a list: level == -1 reads the LAST cell, as the reference's array does
        self.rows = list(range(self.m))
        self.level = 0
        self.frames = []                  # (rows of a scan as a set, cells still alive after it)
        self.memo = {}

    # ---- moves on an explicit state (so that they can be tried on a copy)
    def _next_sibling(self, counter, rows, level):
        for j in [k for k in range(self.N - 1, -1, -1) if counter[k] != 0]:
            level = j
            counter[j] += 1
            if counter[j] <= self.mi[j]:
                rows[-1] -= self.M
                rows.append(self.beg[j] + counter[j] + self.M - 1)
                return level, False
            counter[j] = 0
            del rows[self.m + sum(counter):]
            level = j - 1
            if level == -1:
                return level, True
        return level, False

    def _reopen_after_piece(self, counter, rows, level):
        level -= 1
        for _ in range(sum(1 for c in counter if c != 0)):
            if counter[level] <= self.mi[level]:
                rows[-1] -= self.M
                rows.append(self.beg[level] + counter[level] + self.M)
                return level, False
            counter[level] = 0
            del rows[self.m + sum(counter):]
            if level == -1:
                return level, True
        return level, False

    def _alive(self):
        have = set(self.rows)
        while self.frames and not self.frames[-1][0] <= have:
            self.frames.pop()
        return self.frames[-1][1] if self.frames else list(range(self.N))

    def _radius(self, rows):
        key = tuple(rows)
        if key not in self.memo:
            want = [list(rows)]
            if self.look_ahead:   # the nodes that follow while every node turns out empty, from a copy of the state
                c2, r2, l2 = list(self.counter), list(rows), self.level
                for _ in range(8):
                    if l2 == -1 or c2[l2] == 0:
                        break
                    l2, ended = self._next_sibling(c2, r2, l2)
                    if ended or any(not -self.m - 2 * self.M <= v < self.m + 2 * self.M for v in r2):
                        break
                    want.append(list(r2))
            self.memo.clear()
            for w, rad in zip(want, self.radii_rows(want)):
                self.memo[tuple(w)] = rad if rad == rad else 0   # NaN (no verdict) reads as radius 0 (ref :1294-1297)
        return self.memo[key]

    def run(self):
        N, tol = self.N, self.tol
        while self.level != -1:
            if self.counter[self.level] == 0:
                alive = [j for j in self._alive() if j >= self.level]
                stacks = [self.rows + list(range(self.beg[j], self.beg[j] + self.mi[j])) for j in alive]
                radii = self.radii_rows(stacks) if stacks else []
                # only a cell whose LP was SOLVED with a radius <= tol / 2 stays out of the scans below this node; one
                # without a verdict (NaN: unbounded ball, iteration limit) reads as radius 0 here and is solved again
                self.frames.append((set(self.rows), [j for j, r in zip(alive, radii) if not r <= 0.5 * tol]))
                radii = [r if r == r else 0 for r in radii]
                last = 0   # the reference's R after its loop: the radius of the last cell it looked at
                for j, r in zip(alive, radii):
                    if r > tol:
                        last = r
                        self.level = j
                        self.counter[j] = 1
                        self.rows.append(self.beg[j] + self.M)
                        break
                    if j == N - 1:
                        last = r
                if last < tol:
                    yield 0, list(self.rows)
                    self.level, ended = self._reopen_after_piece(self.counter, self.rows, self.level)
                    if ended:
                        return
            else:
                self.level, ended = self._next_sibling(self.counter, self.rows, self.level)
                if ended:
                    return
            if self._radius(self.rows) > tol:
                if self.level == N - 1:
                    yield 1, list(self.rows)
                else:
                    self.level += 1


# ====================================================================================== volume
def _volume_by_samples(polyreg, nsamples=None, seed=None):
    """volume() of a Polytope with the samples drawn on the host and uploaded: the path of every backend but 'hip', and of
    'hip' where the volume kernel does not apply (more than 64 rows, a box that is not finite, a seed that is neither None
    nor an int)."""
    from .batch import _volume_nsamples
    n = polyreg.A.shape[1]
    N = _volume_nsamples(n, nsamples)   # (the reference's table by dimension and its two ValueErrors, ref :1565-1584)
    l_b, u_b = polyreg.bounding_box
    x = np.tile(l_b, (1, N)) + np.random.default_rng(seed).random((n, N)) * np.tile(u_b - l_b, (1, N))
    # all(A x - b < 0) per sample (ref :1590-1591) == contains(x, abs_tol=0): the containment kernel
    hits = int(np.count_nonzero(_contains_many([polyreg], x, 0.0)))
    vol = np.prod(u_b - l_b) * hits / N
    polyreg._set_volume(vol)
    return vol


def _volume_on_device(poly, nsamples, seed):
    """True when the volume kernel takes this Polytope (polytope_amd.batch.volume_batch): 'hip', within the fused point
    kernels' limits, an integer sample count the kernel holds, a seed that is None or a non-negative int, a finite box.
    Everything else -- the two ValueErrors for `nsamples` among it -- is _volume_by_samples' business."""
    from .batch import _is_int
    if not _use_hip() or not _fits(poly.A.shape[0], poly.A.shape[1]) or poly.A.shape[0] < 1:
        return False
    if nsamples is not None and not (_is_int(nsamples) and 1 <= nsamples <= 2 ** 31 - 1):
        return False
    if seed is not None and not (_is_int(seed) and seed >= 0):
        return False
    l_b, u_b = poly.bounding_box
    return bool(np.all(np.isfinite(l_b)) and np.all(np.isfinite(u_b)))


def _volume_region_hip(region):
    """volume(Region) on 'hip': the members that pass the reference's own gate (is_fulldim(member), ref :1551-1552) and
    that the volume kernel takes go through ONE volume_batch call on the Region's resident rows; the others as before."""
    from . import batch
    members = region.list_poly
    _cheby_fill(members)
    vols = [None] * len(members)
    sel = []
    for k, p in enumerate(members):
        if not is_fulldim(p):
            vols[k] = 0.0          # (its `_volume` stays as it is, as in the reference)
        elif _volume_on_device(p, None, None):
            sel.append(k)
        else:
            vols[k] = _volume_by_samples(p)
    if sel:
        polys = [members[k] for k in sel]
        At, bt, mt = _table_of(polys, region if len(sel) == len(members) else None).dev()
        lb = np.array([p.bbox[0].ravel() for p in polys])
        ub = np.array([p.bbox[1].ravel() for p in polys])
        res = batch.volume_batch(At, bt, m=mt, lb=lb, ub=ub)
        got = res["volume"]
        got = got if isinstance(got, np.ndarray) else got.numpy()
        for k, p, v in zip(sel, polys, got):
            p._set_volume(v)
            vols[k] = v
    tot = 0.0
    for v in vols:
        tot += v
    region._set_volume(tot)
    return tot


def volume(polyreg, nsamples=None, seed=None):
    """Monte-Carlo volume: uniform samples in the bounding box, fraction strictly inside
    (ref :1529-1594).  Region: sum over its members (with the default `nsamples` and `seed=None`, as in the reference).

    On 'hip' the samples -- the ones np.random.default_rng(seed).random((d, N)) draws -- are generated on the device
    (polytope_amd.batch.volume_batch): for a given seed the result is the float the sample-upload path returns.  With
    `seed=None` the members of a Region draw from the spawned children of ONE fresh np.random.SeedSequence, and a single
    Polytope from the one child `np.random.SeedSequence().spawn(1)[0]` -- fresh entropy either way, though not the stream
    np.random.default_rng(None) itself would start."""
    if not is_fulldim(polyreg):
        return 0.0
    if isinstance(polyreg, Region):
        bounding_box(polyreg)  # the members' boxes in one batch of 2d LPs each, cached for the calls below
        if _use_hip():
            return _volume_region_hip(polyreg)
        tot = 0.0
        for p in polyreg.list_poly:
            tot += volume(p)
        polyreg._set_volume(tot)
        return tot
    if not _volume_on_device(polyreg, nsamples, seed):
        return _volume_by_samples(polyreg, nsamples, seed)
    from . import batch
    l_b, u_b = polyreg.bounding_box
    res = batch.volume_batch(polyreg.A[np.newaxis], polyreg.b[np.newaxis], nsamples=nsamples, seed=seed,
                             lb=l_b.reshape(1, -1), ub=u_b.reshape(1, -1))
    vol = res["volume"][0]
    polyreg._set_volume(vol)
    return vol


def volume_exact(poly):
    """The exact volume of one Polytope of dimension <= 4 and at most 64 rows, as a float (polytope_amd.batch.
    volume_exact_batch with reduce=True: 0.0 for an empty or flat polytope, inf for an unbounded one).  Deterministic, and
    apart from `volume`: the cached `poly.volume` (the Monte-Carlo estimate) is neither read nor set.  A Region raises: its
    members may overlap, so their volumes do not add up to the Region's."""
    if isinstance(poly, Region):
        raise Exception("volume_exact: not executable for regions (their members may overlap)")
    from . import batch
    A = np.asarray(poly.A, dtype=float)
    if A.ndim != 2 or A.shape[0] == 0:
        return 0.0   # (the empty Polytope())
    res = batch.volume_exact_batch(A[np.newaxis], np.asarray(poly.b, dtype=float).reshape(1, -1), areas=False)
    return float(res["volume"][0])


# ====================================================================================== nearest points
_NEAREST_BYTES = 256 << 20   # the [P, chunk] buffers of one nearest_batch call over a Region's members stay below this


def _nearest_many(polys, points, owner=None):
    """(x[N, d], dist[N], member int32[N]) over the non-empty descriptions of `polys`: per column of `points` the closest
    point of the union, its distance and the index into `polys` of the member it lies in (the lowest on ties; -1 with
    dist = inf and x = NaN where no member has a point: all empty, or the point is not finite).  'hip' only: one
    batch.nearest_batch per chunk of points, every member against every point of the chunk, and the minimum over the
    members -- on the device when the table is resident there."""
    if not _use_hip():
        raise ValueError("nearest / distance need the 'hip' backend (polytope_amd.batch.nearest_batch), got %r"
                         % (solvers.default_solver,))
    solvers._require("hip")
    points = np.asarray(points, dtype=float)
    if points.ndim != 2:
        raise ValueError("points should be column vectors")
    d, N = points.shape
    idx = np.array([k for k, p in enumerate(polys) if p.A.size > 0], dtype=np.int64)
    x, dist, member = np.full((N, d), np.nan), np.full(N, np.inf), np.full(N, -1, dtype=np.int32)
    if idx.size == 0 or N == 0:
        return x, dist, member
    members = [polys[k] for k in idx]
    if members[0].A.shape[1] != d:
        raise ValueError("points should be column vectors")
    from . import batch
    if len(members) >= 8:
        At, bt, mt = _table_of(members, owner).dev()
    else:
        At, bt, mt = _pack(members)
    P = len(members)
    on_dev = not isinstance(At, np.ndarray)
    torch = _torch_or_none() if on_dev else None
    # per (member, point): dist, x[d], status and the kernel's staging of them
    chunk = max(1, min(N, _NEAREST_BYTES // (P * 8 * (d + 2))))
    pts = np.ascontiguousarray(points.T)
    for lo in range(0, N, chunk):
        X = pts[lo:lo + chunk]
        if on_dev:
            batch._count_h2d(X)
            X = torch.as_tensor(X).to(At.device)
        res = batch.nearest_batch(At, bt, X, m=mt)
        if on_dev:
            dd = torch.where(res["status"] == 0, res["dist"], torch.full_like(res["dist"], float("inf")))
            best, arg = torch.min(dd, dim=0)             # (the first of equal minima is not promised by torch.min:)
            arg = torch.argmax((dd == best[None, :]).to(torch.int8), dim=0)
            xs = res["x"][arg, torch.arange(arg.shape[0], device=arg.device)]
            best, arg, xs = best.cpu().numpy(), arg.cpu().numpy(), xs.cpu().numpy()
        else:
            dd = np.where(res["status"] == 0, res["dist"], np.inf)
            arg = np.argmin(dd, axis=0)
            best = dd[arg, np.arange(arg.size)]
            xs = res["x"][arg, np.arange(arg.size)]
        ok = np.isfinite(best)
        sl = slice(lo, lo + best.size)
        dist[sl] = best
        x[sl] = np.where(ok[:, None], xs, np.nan)
        member[sl] = np.where(ok, idx[arg], -1)
    return x, dist, member


def nearest(polyreg, points):
    """The closest point of a Polytope or Region to every column of `points` ([d, N] column vectors, the convention of
    `contains`).  Polytope -> (x[N, d], dist[N]); Region -> (x[N, d], dist[N], member int32[N]): the minimum over the members,
    the lowest index on ties.  An empty set gives x = NaN, dist = inf (member -1).  Dimension <= 4 and at most 64 rows per
    polytope (batch.nearest_batch; other shapes raise UnsupportedSize); 'hip' backend only."""
    if isinstance(polyreg, Region):
        return _nearest_many(polyreg.list_poly, points, owner=polyreg)
    x, dist, _ = _nearest_many([polyreg], points)
    return x, dist


def distance(polyreg, points):
    """The Euclidean distance of every column of `points` ([d, N]) to a Polytope or Region: nearest(polyreg, points)[1]."""
    return nearest(polyreg, points)[1]


# ====================================================================================== adjacency
def _adjacency_stack(poly1, poly2, overlap, abs_tol):
    """The slightly inflated stacked polytope whose full-dimensionality decides adjacency
    (ref :1855-1885); None when the non-overlap branch can answer False without an LP."""
    A1, A2 = poly1.A.copy(), poly2.A.copy()
    b1, b2 = poly1.b.copy(), poly2.b.copy()
    if overlap:
        b1 += abs_tol
        b2 += abs_tol
    else:
        M1 = np.concatenate((poly1.A, np.array([poly1.b]).T), 1).T
        M1n = np.dot(M1, np.diag(1 / np.sqrt(np.sum(M1 ** 2, 0))))
        M2 = np.concatenate((poly2.A, np.array([poly2.b]).T), 1).T
        M2n = np.dot(M2, np.diag(1 / np.sqrt(np.sum(M2 ** 2, 0))))
        gram = np.dot(M1n.T, M2n)
        if not np.any(gram < -0.99):
            return None
        row, col = np.nonzero(np.isclose(gram, gram.min()))
        for i, j in zip(row, col):
            b1[i] += abs_tol
            b2[j] += abs_tol
    return Polytope(np.concatenate((A1, A2)), np.concatenate((b1, b2)))


def is_adjacent(poly1, poly2, overlap=True, abs_tol=ABS_TOL):
    """True if two polytopes / regions touch (or overlap, with overlap=True): both are inflated
    by abs_tol and the intersection must have Chebyshev radius > abs_tol/10 (ref :1827-1885)."""
    if poly1.dim != poly2.dim:
        raise Exception("is_adjacent: polytopes do not have the same dimension")
    return bool(is_adjacent_pairs([(poly1, poly2)], overlap=overlap, abs_tol=abs_tol)[0])


def is_adjacent_pairs(pairs, overlap=True, abs_tol=ABS_TOL):
    """is_adjacent for many (polytope-or-region, polytope-or-region) pairs; every pair of member
    polytopes contributes one Chebyshev LP and all of them go down as one batch
    (the O(n^2) loop of prop2partition.py:57-61)."""
    stacks, owner = [], []
    result = np.zeros(len(pairs), dtype=bool)
    for k, (pa, pb) in enumerate(pairs):
        if pa.dim != pb.dim:
            raise Exception("is_adjacent: polytopes do not have the same dimension")
        la = pa.list_poly if isinstance(pa, Region) else [pa]
        lb = pb.list_poly if isinstance(pb, Region) else [pb]
        for p in la:
            for q in lb:
                st = _adjacency_stack(p, q, overlap, abs_tol)
                if st is not None:
                    stacks.append(st)
                    owner.append(k)
    for k, r in zip(owner, _radii(stacks) if stacks else []):
        if r > abs_tol / 10:
            result[k] = True
    return result


# ======================================================================================
# Vertex enumeration: qhull / extreme on top of the device-resident
# quickhull of polytope_amd.quickhull and the fused reduce kernel.
def qhull(vertices, abs_tol=ABS_TOL):
    """Convex hull of the rows of `vertices` (N x d) as a Polytope (ref :1685-1695)."""
    from .quickhull import quickhull
    A, b, vert = quickhull(vertices, abs_tol=abs_tol)
    if A.size == 0:
        return Polytope()
    return Polytope(A, b, minrep=True, vertices=vert)


def extreme(poly1):
    """Vertices of a bounded polytope as an (N x d) array, None if it is flat (ref :1597-1682).

    d = 1: b_i / a_i.  d = 2: rows sorted by the angle of their normal, consecutive pairs
    intersected (all 2x2 systems in one batched solve).  d > 2: the facets of the hull of the
    polar dual about the Chebyshev centre are the vertices: qhull of a_i / (b_i - a_i.xc), reduce,
    map back.  Caches the result in `poly1.vertices`.
    """
    if poly1.vertices is not None:
        return poly1.vertices
    if isinstance(poly1, Region):
        raise Exception("extreme: not executable for regions")
    poly1 = reduce(poly1)  # the H-representation must be irredundant
    if not is_fulldim(poly1):
        return None
    A, b = poly1.A.copy(), poly1.b.copy()
    nc, nx = A.shape
    if nx == 1:
        if nc == 1:
            raise Exception("extreme: polytope is unbounded")
        V = b / A[:, 0]
    elif nx == 2:
        order = np.argsort(np.angle(A[:, 0] + 1j * A[:, 1]))
        nxt = np.roll(order, -1)
        HH = np.stack([A[order], A[nxt]], axis=1)   # [nc][2][2]: a facet and its angular successor
        KK = np.stack([b[order], b[nxt]], axis=1)
        if np.any(np.isinf(np.linalg.cond(HH))):
            raise Exception("extreme: polytope is unbounded")
        try:
            V = np.linalg.solve(HH, KK[:, :, None])[:, :, 0]
        except Exception:
            raise Exception("Finding extreme points failed, Check if any unbounded Polytope is causing this.")
    else:
        rmid, xmid = cheby_ball(poly1)
        Ai = A / (b - np.dot(A, xmid))[:, None]
        Q = reduce(qhull(Ai))
        if not is_fulldim(Q):
            return None
        V = Q.A / Q.b[:, None] + np.asarray(xmid).ravel()[None, :]
    a = V.size / nx
    if not float(a).is_integer():
        raise AssertionError(a)
    poly1.vertices = np.asarray(V, dtype=float).reshape((int(a), nx))
    return poly1.vertices


# ====================================================================================== small callers of the path
def is_interior(r0, r1, abs_tol=ABS_TOL):
    """`is_interior` of the reference (ref :1888-1909), whose return value is the opposite of its name: True as soon as some
    member of r1, grown by abs_tol on every facet, sticks out of r0; False when every grown member stays inside.  Kept that way
    (drop-in); the grown members are built with the constructor, as there (rows re-normalised), and tested one at a time in
    order, so the first one that sticks out ends the call."""
    outer = r0 if isinstance(r0, Region) else Region([r0])
    inner = r1.list_poly if isinstance(r1, Region) else [r1]
    return any(not (Polytope(q.A.copy(), q.b.copy() + abs_tol) <= outer) for q in inner)


def separate(reg1, abs_tol=ABS_TOL):
    """Divide a region into connected regions (ref :1795-1824).  The reference grows each component with
    one is_adjacent(component, polytope) call per remaining polytope; a Region is adjacent to a polytope iff
    one of its members is, so all member pairs are tested in ONE batch up front and the greedy pass of the
    reference (same order, same result) runs on that matrix."""
    members = reg1.list_poly
    n = len(members)
    ii, jj = np.tril_indices(n, -1)
    adj = np.eye(n, dtype=bool)
    if n > 1:
        flags = is_adjacent_pairs([(members[i], members[j]) for i, j in zip(ii, jj)])
        adj[ii, jj] = flags
        adj[jj, ii] = flags
    final = []
    left = list(range(n))
    props = reg1.props
    while left:
        comp = [left[0]]
        for j in left[1:]:
            if adj[comp, j].any():
                comp.append(j)
        reg = Region([members[k] for k in comp], [])
        reg.props = props.copy()
        final.append(reg)
        left = [k for k in left if k not in comp]
    return final


def simplices2polytopes(points, triangles):
    """Convert a simplicial mesh to polytopes in H-representation (ref :2419-2439): one qhull per simplex."""
    return [qhull(points[triangle, :]) for triangle in triangles]


# ====================================================================================== projection
def projection(poly1, dim, solver=None, abs_tol=ABS_TOL, verbose=0):
    """Projection of a polytope onto the coordinates `dim` (1-based), ref :1698-1794.

    Solvers: "fm" (Fourier-Motzkin), "exthull" (vertex projection), "iterhull" (iterative hull), "esp" (needs glpk, which
    is not available: raises).  Without one (or with an unknown name, which logs a warning) the reference's choice:
    <= 2 deleted dimensions fm, <= 4 dimensions exthull, else iterhull.  On 'hip' the fm steps run on the device
    (polytope_amd.batch: the Fourier-Motzkin step kernels and the fused reduce); the existence LP and everything before
    it (the early return, the zero-padding of a polytope with fewer rows than dimensions, which is written back into
    `poly1`) as in the reference."""
    if isinstance(poly1, Region):
        ret = Polytope()
        for i in range(len(poly1.list_poly)):
            p = projection(poly1.list_poly[i], dim, solver=solver, abs_tol=abs_tol)
            ret = ret + p   # (Polytope has no `+`: TypeError, as in the reference)
        return ret
    if (poly1.dim < len(dim)) or is_empty(poly1):
        return poly1
    poly_dim = poly1.dim
    dim = np.array(dim)
    org_dim = range(poly_dim)
    new_dim = dim.flatten() - 1
    del_dim = np.setdiff1d(org_dim, new_dim)
    mA, nA = poly1.A.shape
    if mA < poly_dim:
        logger.warning("fewer rows in A: " + str(mA) + ", than polytope dimension: " + str(poly_dim))
        A = poly1.A.copy()
        poly1.A = np.zeros((poly_dim, poly_dim))
        poly1.A[0:mA, 0:nA] = A
        poly1.b = np.hstack([poly1.b, np.zeros(poly_dim - mA)])
    # does the projection exist: a Chebyshev-style LP with the squared norms, zeroed on the ROWS del_dim (ref :1757-1769)
    norm = np.sum(poly1.A * poly1.A, axis=1).flatten()
    norm[del_dim] = 0
    c = np.zeros(len(org_dim) + 1, dtype=float)
    c[len(org_dim)] = -1
    G = np.hstack([poly1.A, norm.reshape(norm.size, 1)])
    h = poly1.b
    sol = lpsolve(c, G, h)
    if sol["status"] != 0:
        return Polytope()
    if sol["x"][-1] < abs_tol:
        return Polytope()
    if solver == "esp":
        return projection_esp(poly1, new_dim, del_dim)
    elif solver == "exthull":
        return projection_exthull(poly1, new_dim)
    elif solver == "fm":
        return projection_fm(poly1, new_dim, del_dim)
    elif solver == "iterhull":
        return projection_iterhull(poly1, new_dim)
    elif solver is not None:
        logger.warning('unrecognized projection solver "' + str(solver) + '".')
    if len(del_dim) <= 2:
        return projection_fm(poly1, new_dim, del_dim)
    elif len(org_dim) <= 4:
        return projection_exthull(poly1, new_dim)
    else:
        return projection_iterhull(poly1, new_dim)


def _fm_combine_host(poly, i, abs_tol=ABS_TOL):
    """One elimination of projection_fm as the reference writes it (ref :1925-1948): P x Q combinations through np.dot."""
    positive = np.nonzero(poly.A[:, i] > abs_tol)[0]
    negative = np.nonzero(poly.A[:, i] < -abs_tol)[0]
    null = np.nonzero(np.abs(poly.A[:, i]) < abs_tol)[0]
    nr = len(null) + len(positive) * len(negative)
    nc = np.shape(poly.A)[0]
    C = np.zeros([nr, nc])
    A = poly.A[:, i].copy()
    row = 0
    for j in positive:
        for k in negative:
            C[row, j] = -A[k]
            C[row, k] = A[j]
            row += 1
    for j in null:
        C[row, j] = 1
        row += 1
    keep_dim = np.setdiff1d(range(poly.A.shape[1]), np.array([i]))
    return Polytope(np.dot(C, poly.A)[:, keep_dim], np.dot(C, poly.b))


def _fm_eliminate_dev(poly, i, first, abs_tol=ABS_TOL):
    """The same elimination on the device (B = 1; csrc/plp_fm.hip) from the rows of `poly` as they stand; `first`: one
    constructor pass before (the copy() of the first step)."""
    from .batch import fm_count, fm_emit
    A = np.ascontiguousarray(poly.A, dtype=float)[None]
    b = np.ascontiguousarray(poly.b, dtype=float)[None]
    n = int(fm_count(A, b, int(i), first=first, abs_tol=abs_tol)[0])
    Ao, bo, mo = fm_emit(A, b, int(i), max(n, 1), first=first, abs_tol=abs_tol)
    k = int(mo[0])
    return Polytope(Ao[0, :k], bo[0, :k], normalize=False)


def _fm_dev_fits(poly):
    from .batch import MAX_D
    return poly.A.ndim == 2 and 2 <= poly.A.shape[1] <= MAX_D and poly.A.shape[0] >= 1 and np.all(np.isfinite(poly.b))


def _fm_host_continue(poly, cols, abs_tol, start):
    """projection_fm from the middle, per polytope: `start` "reduce" -- `poly` is an elimination's output (is_fulldim,
    reduce, then the columns `cols`); None -- `poly` is the input (reduce, copy, then `cols`).  Eliminations on the
    device as in the batch, reductions through reduce()."""
    if start is None:
        poly = reduce(poly)
        poly.A[:, cols[0]] if len(cols) else None   # (reduce() returned Polytope(): IndexError, as the reference)
        first = True
    else:
        if not is_fulldim(poly):
            return Polytope()
        poly = reduce(poly)
        first = False
    for i in cols:
        poly = _fm_eliminate_dev(poly, i, first, abs_tol)
        first = False
        if not is_fulldim(poly):
            return Polytope()
        poly = reduce(poly)
    if first:
        poly = poly.copy()
    return poly


def projection_fm(poly1, new_dim, del_dim, abs_tol=ABS_TOL):
    """Fourier-Motzkin elimination of the columns del_dim, the last first (ref :1911-1952).  On 'hip' the steps are the
    device driver of polytope_amd.batch with one polytope; otherwise the reference's loop over reduce() / is_fulldim()."""
    del_dim = -np.sort(-np.asarray(del_dim))
    if not poly1.minrep:
        poly1 = reduce(poly1)
    if _use_hip() and _fm_dev_fits(poly1):
        return _projection_fm_dev(poly1, [int(i) for i in del_dim], abs_tol)
    poly = poly1.copy()
    for i in del_dim:
        poly = _fm_combine_host(poly, i, abs_tol)
        if not is_fulldim(poly):
            return Polytope()
        poly = reduce(poly)
    return poly


def _projection_fm_dev(poly1, cols, abs_tol):
    import torch
    from .batch import _fm_batch, PROJ_OK, PROJ_RAISES, PROJ_LPFAIL
    if not cols:
        return poly1.copy()
    dev = torch.device("cuda", torch.cuda.current_device())
    m, d = poly1.A.shape
    A = torch.as_tensor(np.ascontiguousarray(poly1.A, dtype=float)[None], device=dev)
    b = torch.as_tensor(np.ascontiguousarray(poly1.b, dtype=float)[None], device=dev)
    mt = torch.full((1,), m, dtype=torch.int32, device=dev)
    host = {}

    def on_host(k, poly, cols_left, start):
        host[k] = _fm_host_continue(poly, cols_left, abs_tol, start)
    res = _fm_batch(A, b, mt, cols, abs_tol, [True], on_host)
    if res[1] is not None:   # finished in the last step
        _, Ao, bo, mo, minrep = res[1]
        return Polytope(Ao[0, :mo[0]], bo[0, :mo[0]], minrep=bool(minrep[0]), normalize=False)
    if res[0] is None:
        return host[0]
    st, Ao, bo, minrep = res[0]
    if st == PROJ_LPFAIL:
        raise RuntimeError("bounding_box: an LP of the box prefilter of `reduce` ended with status 1 or 4")
    if st == PROJ_RAISES:
        raise IndexError("too many indices for array: array is 1-dimensional, but 2 were indexed")
    if st != PROJ_OK:
        return Polytope()
    return Polytope(Ao, bo, minrep=bool(minrep), normalize=False)


def projection_exthull(poly1, new_dim):
    """Vertex projection (ref :1955-1965): the hull of the projected vertices, reduced."""
    vert = extreme(poly1)
    if vert is None:
        return Polytope(fulldim=False, minrep=True)
    return reduce(qhull(vert[:, new_dim]))


def _iterhull_lp_failed(sol):
    raise RuntimeError(("`polytope.solvers.lpsolve` returned:  {v}\n"
                        "its docstring describes return values").format(v=sol))


def projection_iterhull(poly1, new_dim, max_iter=1000, verbose=0, abs_tol=ABS_TOL):
    """Iterative hull (ref :1968-2098): the same random directions from np.random in the same order, the same rounded
    cache keys; the facet LPs of one iteration that the cache does not answer go down as one batch (lpsolve_many), each
    key once -- what the reference's loop, which fills the cache as it goes, solves."""
    r, xc = cheby_ball(poly1)
    org_dim = poly1.A.shape[1]
    if len(new_dim) == 1:
        f1 = np.zeros(poly1.A.shape[1])
        f1[new_dim] = 1
        sol = lpsolve(f1, poly1.A, poly1.b)
        if sol["status"] != 0:
            _iterhull_lp_failed(sol)
        vert1 = sol["x"]
        sol = lpsolve(np.negative(f1), poly1.A, poly1.b)
        if sol["status"] != 0:
            _iterhull_lp_failed(sol)
        vert2 = sol["x"]
        return qhull(np.vstack([vert1, vert2]), abs_tol=abs_tol)
    OK = False
    cnt = 0
    Vert = None
    while not OK:
        cnt += 1
        if cnt > max_iter:
            raise Exception("iterative_hull: could not find starting simplex")
        f1 = np.random.rand(len(new_dim)).flatten() - 0.5
        f = np.zeros(org_dim)
        f[new_dim] = f1
        sol = lpsolve(np.negative(f), poly1.A, poly1.b)
        xopt = np.array(sol["x"]).flatten()
        if Vert is None:
            Vert = xopt.reshape(1, xopt.size)
        else:
            k = np.nonzero(Vert[:, new_dim[0]] == xopt[new_dim[0]])[0]
            for j in new_dim[range(1, len(new_dim))]:
                ii = np.nonzero(Vert[k, j] == xopt[j])[0]
                k = k[ii]
                if k.size == 0:
                    break
            if k.size == 0:
                Vert = np.vstack([Vert, xopt])
        if Vert.shape[0] > len(new_dim):
            u, s, v = np.linalg.svd(np.transpose(Vert[:, new_dim] - Vert[0, new_dim]))
            rank = np.sum(s > abs_tol * 10)
            if rank == len(new_dim):
                OK = True
    cnt = 0
    P1 = qhull(Vert[:, new_dim], abs_tol=abs_tol)
    HP = None
    while True:
        cnt += 1
        if cnt > max_iter:
            raise Exception("iterative_hull: maximum number of iterations reached")
        seen = set() if HP is None else {tuple(row) for row in HP[:, :P1.A.shape[1] + 1]}
        todo = []   # (f1, f2) of the facets whose key is neither cached nor already asked for in this iteration
        for ind in range(P1.A.shape[0]):
            f1 = np.round(P1.A[ind, :] / abs_tol) * abs_tol
            f2 = np.hstack([np.round(P1.A[ind, :] / abs_tol) * abs_tol, np.round(P1.b[ind] / abs_tol) * abs_tol])
            key = tuple(f2)
            if key in seen:
                continue
            seen.add(key)
            todo.append((f1, f2))
        cs = []
        for f1, _ in todo:
            f = np.zeros(poly1.A.shape[1])
            f[new_dim] = f1
            cs.append(np.negative(f))
        sols = solvers.lpsolve_many(cs, [poly1.A] * len(cs), [poly1.b] * len(cs))
        for (f1, f2), sol in zip(todo, sols):
            if sol["status"] != 0:
                logger.error("iterhull: LP failure")
                seen.discard(tuple(f2))
                continue
            xopt = np.array(sol["x"]).flatten()
            add = np.hstack([f2, np.round(xopt / abs_tol) * abs_tol])
            HP = add.reshape(1, add.size) if HP is None else np.vstack([HP, add])
            Vert = np.vstack([Vert, xopt])
        P2 = qhull(Vert[:, new_dim], abs_tol=abs_tol)
        OK = 1
        for i in range(np.shape(Vert)[0]):
            if not P1.contains(np.transpose([Vert[i, new_dim]]), abs_tol=abs_tol):
                OK = 0
                break
        if OK == 1:
            return P2
        P1 = P2


def projection_esp(poly1, keep_dim, del_dim):
    """Equality set projection (ref :2101-2114, esp.py): needs glpk, which this package does not bind."""
    if "glpk" not in solvers.installed_solvers:
        raise Exception("projection_esp error: Equality set projection requires `cvxopt.glpk` to run.")
    raise Exception("projection_esp: not provided")


# ====================================================================================== distances between cells
def distance_pairs(cells, pairs):
    """(dist[K], x[K, d], y[K, d]) for the listed pairs (i, j) of a list of Polytopes: the Euclidean distance of cells[i] and
    cells[j] and a closest pair of points, x in cells[i] and y in cells[j] (dist = 0 where they meet).  dist = inf and NaN
    points where a cell is empty; NaN throughout where the call could not settle a pair (an unbounded cell, no
    convergence).  ONE batch.distance_pairs call on the cells' packed table (kept by _table_of, as intersect_pairs does).
    Dimension <= 4 and at most 64 rows per cell (other shapes raise UnsupportedSize); 'hip' backend only."""
    if not _use_hip():
        raise ValueError("distance_pairs / set_distance need the 'hip' backend (polytope_amd.batch.distance_pairs), got %r"
                         % (solvers.default_solver,))
    solvers._require("hip")
    cells = list(cells)
    plist = np.array([(int(i), int(j)) for i, j in pairs], dtype=np.int64).reshape(-1, 2)
    K = plist.shape[0]
    if K and (plist.min() < 0 or plist.max() >= len(cells) or np.any(plist[:, 0] == plist[:, 1])):
        raise ValueError("distance_pairs: pairs must name two different cells of [0, %d)" % len(cells))
    dims = {c.A.shape[1] for c in cells if c.A.size}
    if len(dims) > 1:
        raise ValueError("distance_pairs: cells of different dimensions")
    d = dims.pop() if dims else 0
    dist, x, y = np.full(K, np.inf), np.full((K, d), np.nan), np.full((K, d), np.nan)
    slot = {k: s for s, k in enumerate(k for k, c in enumerate(cells) if c.A.size)}
    at = np.array([t for t in range(K) if plist[t, 0] in slot and plist[t, 1] in slot], dtype=np.int64)
    if not at.size:
        return dist, x, y
    from . import batch
    members = [cells[k] for k in slot]
    if len(members) >= 8:
        At, bt, mt = _table_of(members).dev()
    else:
        At, bt, mt = _pack(members)
    listed = np.array([(slot[plist[t, 0]], slot[plist[t, 1]]) for t in at], dtype=np.int32)
    if not isinstance(At, np.ndarray):
        batch._count_h2d(listed)
        listed = _torch_or_none().as_tensor(listed).to(At.device)
    res = batch.distance_pairs(At, bt, listed, m=mt)
    res = {k: (v if isinstance(v, np.ndarray) else v.cpu().numpy()) for k, v in res.items()}
    st = res["status"]
    dist[at] = np.where(st == 0, res["dist"], np.where(st == 2, np.inf, np.nan))
    x[at], y[at] = res["x"], res["y"]
    return dist, x, y


def set_distance(a, b):
    """The Euclidean distance of two sets, each a Polytope or a Region: the minimum over all member pairs, from one
    distance_pairs call.  -> (dist, x[d], y[d], (member_a, member_b)): a closest pair of points, x in `a` and y in `b`, and
    the members they lie in (indices into list_poly; 0 for a Polytope); the lowest pair index wins ties, pairs counted
    member_a-major.  (inf, NaN, NaN, (-1, -1)) where no pair has a distance: a set is empty."""
    la = a.list_poly if isinstance(a, Region) else [a]
    lb = b.list_poly if isinstance(b, Region) else [b]
    na, nb = len(la), len(lb)
    pairs = [(i, na + j) for i in range(na) for j in range(nb)]
    dist, x, y = distance_pairs(list(la) + list(lb), pairs)
    d = x.shape[1]
    if not len(pairs) or not np.any(np.isfinite(dist)):
        return np.inf, np.full(d, np.nan), np.full(d, np.nan), (-1, -1)
    t = int(np.argmin(np.where(np.isfinite(dist), dist, np.inf)))
    return float(dist[t]), x[t].copy(), y[t].copy(), (t // nb, t % nb)
