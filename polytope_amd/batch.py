"""Batched entry points of the MI355X engine (no counterpart in the reference, which loops
in Python: polytope/polytope.py:1142-1151, :1367-1409, :2148-2152, prop2partition.py:57-61).

Every function takes either numpy arrays (host path: the C ABI copies in and out and
blocks) or torch CUDA tensors (device path: pointers are handed to the `_dev` entry points
on torch's current stream, results come back as CUDA tensors, nothing synchronises).

Packing: A[B, m_max, d], b[B, m_max], optional int32 m[B] (rows used per polytope).
"""
import ctypes as C
import sys
import time

import numpy as np

from . import _lib

MAX_M, MAX_D = 64, 16


def _is_torch(x):
    return type(x).__module__.startswith("torch")


def _np(a, dtype=np.float64):
    return np.ascontiguousarray(a, dtype=dtype)


def _ptr(a):
    if a is None:
        return None
    if _is_torch(a):
        return C.c_void_p(a.data_ptr())
    return C.c_void_p(a.ctypes.data)


def _finite_or_raise(what, *arrays):
    for a in arrays:
        if a is not None and not np.all(np.isfinite(a)):
            # same exception class scipy.optimize.linprog raises on inf/nan input
            raise ValueError("%s: input must not contain values inf, nan, or None" % what)


# Debug counter: bytes the host-pointer entry points of this module handed to the library for upload (and the bytes
# polytope_amd.polytope moved to the device when it made a packed table resident).  Device-pointer calls add nothing.
h2d_bytes = 0


def _count_h2d(*arrays):
    global h2d_bytes
    for a in arrays:
        if a is not None:
            h2d_bytes += int(a.nbytes)


def _torch_stream_ctx(t):
    import torch
    dev = t.device.index if t.device.index is not None else torch.cuda.current_device()
    ctx = _lib.context(dev)
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    return torch, ctx, stream


def _tprep(torch, t, dtype):
    if t is None:
        return None
    if t.dtype != dtype or not t.is_contiguous():
        t = t.to(dtype).contiguous()
    return t


_SCALARS = (int, float)
_TORCH_DTYPE = {}


def _torch_dtypes(torch):
    """numpy dtype -> torch dtype.  torch has no unsigned words: keep masks and hit counts are the same bits in the signed type."""
    if not _TORCH_DTYPE:
        _TORCH_DTYPE.update({np.float64: torch.float64, np.int32: torch.int32, np.int64: torch.int64, np.uint8: torch.uint8,
                             np.uint32: torch.int32, np.uint64: torch.int64})
    return _TORCH_DTYPE


class _Backend:
    """Where the arrays of one call live, chosen from its first array: numpy (the host-pointer entry point `name`, which
    copies in and out on the context's stream and blocks) or torch CUDA tensors (`name + "_dev"` on torch's current stream;
    nothing synchronises).  A public function states its shapes, dtypes and argument order once, in terms of this object."""

    def __init__(self, first):
        # (nothing of the library is touched before call(): argument errors are raised without it)
        self.torch = None
        if _is_torch(first):
            self.torch = sys.modules["torch"]
            self.first, self.device, self.dtypes = first, first.device, _torch_dtypes(self.torch)

    def arr(self, a, dtype=np.float64, shape=None):
        """An input, contiguous and of `dtype` (None stays None); a numpy input is also brought to `shape`."""
        if a is None:
            return None
        if self.torch is not None:
            return _tprep(self.torch, a, self.dtypes[dtype])
        a = _np(a, dtype)
        return a if shape is None else a.reshape(shape)

    def out(self, shape, dtype=np.float64, zero=False):
        """An output.  `zero`: a numpy output the library may leave unwritten (an empty call returns before any copy)."""
        if self.torch is not None:
            return self.torch.empty(shape, dtype=self.dtypes[dtype], device=self.device)
        return (np.zeros if zero else np.empty)(shape, dtype)

    def call(self, name, *args, h2d=()):
        """The entry point `name` of this backend with `args` (arrays as pointers) behind the context (and the stream).
        `h2d`: the numpy inputs whose upload the debug counter is to see."""
        lib = _lib.load()
        if self.torch is not None:   # (sizes and tolerances go as they are)
            name += "_dev"
            _, ctx, stream = _torch_stream_ctx(self.first)
            args = [a if a.__class__ in _SCALARS else None if a is None else C.c_void_p(a.data_ptr()) for a in args]
            rc = getattr(lib, name)(ctx.handle, stream, *args)
        else:
            _count_h2d(*h2d)
            args = [a if a.__class__ in _SCALARS else None if a is None else C.c_void_p(a.ctypes.data) for a in args]
            rc = getattr(lib, name)(_lib.context().handle, *args)
        if rc:
            _lib.check(rc, name)


def _packed(be, A, b, m, name="A"):
    """The packed table every batch takes -> A[B, m_max, d], b[B, m_max], m int32[B] or None, (B, m_max, d)."""
    A = be.arr(A)
    if len(A.shape) != 3:
        raise ValueError("%s must be [B, m_max, %s]" % (name, "n" if name == "G" else "d"))
    B, m_max, d = A.shape
    return A, be.arr(b, shape=(B, m_max)), be.arr(m, np.int32, (B,)), (B, m_max, d)


# --------------------------------------------------------------------------------------
def lpsolve_batch(c, G, h, m=None):
    """B independent LPs  min c'x s.t. Gx <= h, x free  (solvers.py:76-106 semantics per LP).

    c[B,n], G[B,m_max,n], h[B,m_max] -> dict(status int32[B], x[B,n], fun[B], iters int32[B]);
    x/fun are NaN where status != 0.
    """
    be = _Backend(G)
    G, h, m, (B, m_max, n) = _packed(be, G, h, m, "G")
    c = be.arr(c, shape=(B, n))
    # (inf / nan in numpy inputs: ValueError from the library, which checks them while staging -- plp_ctx_set_check_finite)
    x, fun = be.out((B, n)), be.out((B,))
    status, iters = be.out((B,), np.int32), be.out((B,), np.int32)
    be.call("plp_lp_solve_batch", B, m_max, n, c, G, h, m, x, fun, status, iters, h2d=(c, G, h, m))
    return dict(status=status, x=x, fun=fun, iters=iters)


def cheby_ball_batch(A, b, m=None):
    """Chebyshev-ball LP (F1, polytope.py:1283-1288) of B polytopes.

    -> dict(r[B] raw x[-1], xc[B,d], status[B]).  cheby_ball's own post-processing
    (status != 0 or r < 0 -> (0, None), :1289-1297) is left to the caller.
    """
    be = _Backend(A)
    A, b, m, (B, m_max, d) = _packed(be, A, b, m)
    # (inf / nan in numpy inputs: ValueError from the library, which checks them while staging -- plp_ctx_set_check_finite)
    r, xc, status = be.out((B,)), be.out((B, d)), be.out((B,), np.int32)
    be.call("plp_cheby_batch", B, m_max, d, A, b, m, r, xc, status, h2d=(A, b, m))
    return dict(r=r, xc=xc, status=status)


def bbox_batch(A, b, m=None):
    """Bounding boxes of B polytopes with 1 <= d <= 16 (bounding_box's LP loops, polytope.py:1367-1409): the
    Chebyshev LP and 2d LPs from its centre per polytope, one launch.

    -> dict(lb[B,d], ub[B,d], status[B]): status 0 = box valid (+-inf where unbounded), 1 = polytope not handled
    here (no centre with r >= 1e-6, or a Bland case): the caller solves the 2d generic LPs for it.
    """
    be = _Backend(A)
    A, b, m, (B, m_max, d) = _packed(be, A, b, m)
    # (inf / nan in numpy inputs: ValueError from the library, which checks them while staging -- plp_ctx_set_check_finite)
    lb, ub, status = be.out((B, d)), be.out((B, d)), be.out((B,), np.int32)
    be.call("plp_bbox_batch", B, m_max, d, A, b, m, lb, ub, status, h2d=(A, b, m))
    return dict(lb=lb, ub=ub, status=status)


def reduce_batch(A, b, m=None, abs_tol=1e-7, out=None):
    """Fused reduce() (polytope.py:1053-1163) of B non-minrep polytopes.

    -> dict(keep uint64[B] (bit i = input row i kept), flags int32[B] (RF_*), r[B], xc[B,d],
            nlp int32[B] = LPs the reference would have issued for that polytope)
    Polytopes of more than 64 rows (m_max > 64; the reference has no row limit): keep is [B, W], W = ceil(m_max / 64)
    words per polytope (plp_reduce_wide_batch; `keep_to_bool` reads either shape).
    `out` (device path only): a dict of preallocated, contiguous CUDA tensors keep int64[B], flags
    int32[B], r float64[B], xc float64[B,d], nlp int32[B] to write into (e.g. views of one exchange buffer,
    polytope_amd.dist.ResultBuffer).
    """
    be = _Backend(A)
    A, b, m, (B, m_max, d) = _packed(be, A, b, m)
    # (inf / nan in numpy inputs: ValueError from the library, which checks them while staging -- plp_ctx_set_check_finite)
    wide = m_max > 64
    want = (("keep", np.uint64, (B, (m_max + 63) // 64) if wide else (B,)), ("flags", np.int32, (B,)),
            ("r", np.float64, (B,)), ("xc", np.float64, (B, d)), ("nlp", np.int32, (B,)))
    if be.torch is None or out is None:
        res = {k: be.out(shp, dt) for k, dt, shp in want}
    elif wide:
        raise ValueError("reduce_batch: `out` is for polytopes of up to 64 rows (one keep word each)")
    else:
        res = {k: out[k] for k, _, _ in want}
        for k, dt, shp in want:
            t = res[k]
            if (t.dtype != be.dtypes[dt] or tuple(t.shape) != shp or not t.is_contiguous()
                    or t.device != A.device):
                raise ValueError("reduce_batch: `out` tensors must be contiguous CUDA tensors of the documented "
                                 "dtype and shape")
    be.call("plp_reduce_wide_batch" if wide else "plp_reduce_batch", B, m_max, d, A, b, m, float(abs_tol),
            res["keep"], res["flags"], res["r"], res["xc"], res["nlp"], h2d=(A, b, m))
    return res


def _ctx_and_stream(device, stream):
    """The context of `device` and the stream handle a counter query runs on: `stream` (a torch stream), by default torch's
    current stream when torch is loaded with a GPU, else NULL (the HIP default stream)."""
    ctx = _lib.context(device)
    if stream is None:
        torch = sys.modules.get("torch")
        if torch is not None and torch.cuda.is_available():
            stream = torch.cuda.current_stream(ctx.device)
    return ctx, C.c_void_p(stream.cuda_stream) if stream is not None else None


def reduce_simplex_runs(device=None, reset=False, stream=None):
    """Number of LPs that ran the simplex in the fused reduce launches of this process's context for `device` since the
    counter was last reset (include/plp.h: plp_reduce_counters) -- `nlp` counts the LPs the reference issues, of which
    the presolve settles a part without a simplex run.  The first call switches the counting on and returns 0.
    `stream`: a torch stream (default: torch's current stream when torch is loaded with a GPU, else the HIP default)."""
    lib = _lib.load()
    ctx, sp = _ctx_and_stream(device, stream)
    out = C.c_uint64(0)
    _lib.check(lib.plp_reduce_counters(ctx.handle, sp, C.cast(C.byref(out), C.c_void_p), 1 if reset else 0),
               "plp_reduce_counters")
    return int(out.value)


def verify_careful_lps(device=None, stream=None):
    """How many LPs of the LAST lpsolve_batch / cheby_ball_batch / bbox_batch call did not pass the verifier's certificate (or
    were reported unbounded / at a limit) and were solved again by the careful double-double engine (include/plp.h:
    plp_verify_counters).  `stream`: a torch stream (default: torch's current stream when torch is loaded with a GPU; calls
    with numpy arrays run on the context's own stream, which the library falls back to).  Blocks until that batch is done."""
    lib = _lib.load()
    ctx, sp = _ctx_and_stream(device, stream)
    out = C.c_int64(0)
    _lib.check(lib.plp_verify_counters(ctx.handle, sp, C.cast(C.byref(out), C.c_void_p)), "plp_verify_counters")
    return int(out.value)


def lp_histograms(result):
    """Status and pivot-count histograms of an lpsolve_batch result (counters): dict(status={code: count},
    iters=(edges, counts) over the engines' pivot counts -- LPs the careful engine re-solved keep the engine's count)."""
    st = result["status"]
    it = result.get("iters")
    st = st.cpu().numpy() if hasattr(st, "cpu") else np.asarray(st)
    codes, cnt = np.unique(st, return_counts=True)
    out = {"status": {int(c): int(n) for c, n in zip(codes, cnt)}}
    if it is not None:
        it = it.cpu().numpy() if hasattr(it, "cpu") else np.asarray(it)
        edges = np.array([0, 1, 2, 4, 8, 16, 32, 64, 128, 256, 1 << 30])
        out["iters"] = (edges.tolist(), np.histogram(it, bins=edges)[0].tolist())
    return out


def keep_to_bool(keep, m_max):
    """uint64 keep masks (one word per polytope, or [B, W] words for more than 64 rows) -> bool[B, m_max]."""
    keep = np.asarray(keep).astype(np.uint64)
    if keep.ndim == 1:
        keep = keep[:, None]
    rows = np.arange(m_max)
    words = keep[:, rows // 64]
    return ((words >> (rows % 64).astype(np.uint64)[None, :]) & np.uint64(1)).astype(bool)


def contains_batch(A, b, X, abs_tol=1e-7, m=None, region=True):
    """Containment of the N column vectors X[d, N] in P polytopes (polytope.py:206-218, :732-746).

    region=True  -> uint8[N]    OR over the polytopes (Region.contains; all P*N tests evaluated)
    region=False -> uint8[P, N] one row per polytope (Polytope.contains)
    """
    be = _Backend(X)
    A, b, m, (P, m_max, d) = _packed(be, A, b, m)
    X = be.arr(X)
    if len(X.shape) != 2 or X.shape[0] != d:
        raise ValueError("points should be column vectors")
    N = X.shape[1]
    out = be.out((N,) if region else (P, N), np.uint8, zero=True)
    be.call("plp_contains", P, m_max, d, A, b, m, N, X, float(abs_tol), 0 if region else 1, out, h2d=(A, b, m, X))
    return out


# ------------------------------------------------------------------------------------- point location
# Relative pad of a polytope's box before it is cut into cells: max(1e-9, 1000 x the worst excess of a dense-accepted point
# beyond the oracle's box of the normalised relaxed rows over the soak families) -- DESIGN 4.15 has the measurement
# (scripts/measure_locate_pad.py: worst 3.16e-12, in the `dup` family; at the rounding level, <= 2e-16, in the others).
_LOCATE_PAD = 3.2e-9
_LOCATE_MAX_CELLS = 1 << 18    # include/plp.h: PLP_LOCATE_MAX_CELLS
_LOCATE_MAX_ITEMS = 1 << 24    # entries of cell_items beyond which a grid is declined
_LOCATE_MAX_LIST = 1024        # ... and the longest single list
_LOCATE_MAX_RES = 4096         # cells along one axis
# grid="auto": dense below this many polytopes.  Measured (P sweep at N = 2^20, square cells in d = 2, grid build
# included): dense 0.31 / 1.19 ms at P = 256 / 1024 against 0.70 / 0.65 ms -- the crossing is near P = 600.
_LOCATE_AUTO_P = 600


class _HostStruct(object):
    """A ctypes structure as an argument of _Backend.call: a host pointer on either backend."""

    def __init__(self, obj):
        self.obj = obj
        self.data = C.addressof(obj)
        self.ctypes = self

    def data_ptr(self):
        return self.data


class LocateGrid(object):
    """What locate_grid builds for one packed table and one abs_tol: kind "grid" with the descriptor (axes, lo, inv_h, res)
    and the cell lists cell_start int32[G + 1], cell_items int32[n_items] (numpy, or resident CUDA tensors), or kind
    "dense" -- the grid was declined (`reason` says why) and locate_batch runs the dense kernel."""

    def __init__(self, kind, abs_tol, shape, desc=None, cell_start=None, cell_items=None, n_items=0, max_list=0,
                 pad=_LOCATE_PAD, reason=""):
        self.kind, self.abs_tol, self.shape = kind, float(abs_tol), tuple(int(v) for v in shape)
        self.desc, self.cell_start, self.cell_items = desc, cell_start, cell_items
        self.n_items, self.max_list, self.pad, self.reason = int(n_items), int(max_list), float(pad), reason

    @property
    def axes(self):
        return [] if self.desc is None else [int(self.desc.axis[j]) for j in range(self.desc.naxes)]

    @property
    def res(self):
        return [] if self.desc is None else [int(self.desc.res[j]) for j in range(self.desc.naxes)]

    @property
    def cells(self):
        return int(np.prod(self.res)) if self.desc is not None else 0

    def __repr__(self):
        if self.kind != "grid":
            return "LocateGrid(dense: %s)" % self.reason
        return "LocateGrid(axes=%s, res=%s, items=%d, longest list=%d)" % (self.axes, self.res, self.n_items, self.max_list)


def _locate_axes(P, dom_lo, dom_hi, wsum, nfin, d):
    """The gridded axes and their resolutions from per-axis statistics of the boxes (host scalars): over the polytopes whose
    box is finite on axis k, dom_lo / dom_hi = the extent of the boxes, wsum = the sum of their widths, nfin = how many.
    A cell is about as wide as the mean box; the min(d, 3) axes along which a polytope covers the smallest share of the
    cells are taken; the product of the resolutions is capped at max(64, 8 P) and 2^18.  -> [(axis, lo, inv_h, res)]"""
    cand = []
    for k in range(d):
        ext = dom_hi[k] - dom_lo[k]
        if not (nfin[k] > 0 and np.isfinite(ext) and ext > 0):
            continue
        wmean = wsum[k] / nfin[k]
        res = int(min(_LOCATE_MAX_RES, max(1.0, np.floor(ext / max(wmean, ext / _LOCATE_MAX_RES) + 0.5))))
        if res < 2:
            continue
        cover = (nfin[k] * min(1.0, wmean / ext + 1.0 / res) + (P - nfin[k])) / float(P)
        cand.append((cover, k, float(dom_lo[k]), float(ext), res))
    cand.sort()
    cand = cand[:min(d, 3)]
    if not cand:
        return []
    # cell 0 starts half a cell below the boxes: a tiling whose cells line up with the grid's would otherwise touch three
    # cells per axis (its own and, by the relaxation and the pad, both neighbours) instead of two
    cap = min(_LOCATE_MAX_CELLS, max(64, 8 * P))
    res = [c[4] for c in cand]
    while int(np.prod([r + 1 for r in res])) > cap:
        j = int(np.argmax(res))
        res[j] = max(1, res[j] * 3 // 4)
    return [(k, lo - 0.5 * ext / r, r / ext, r + 1) for (_, k, lo, ext, _), r in zip(cand, res)]


def _locate_rows(be, A, b, m, abs_tol):
    """The relaxed, normalised rows of locate_grid on the backend of A -> An, bn (vacuous, unusable and padding rows become
    0 . x <= 1), every[P] (no box to be had from these rows: listed everywhere), nowhere[P] (contains nothing)."""
    tor = be.torch
    xp = tor if tor is not None else np
    kw = {} if tor is None else {"device": be.device}
    P, m_max = int(A.shape[0]), int(A.shape[1])
    with np.errstate(all="ignore"):
        rows = (xp.arange(m_max, **kw)[None, :] < m[:, None]) if m is not None else \
            xp.ones((P, m_max), dtype=(bool if tor is None else tor.bool), **kw)
        nrm = xp.sqrt((A * A).sum(-1))
        br = b + abs_tol
        zero = rows & (A == 0).all(-1)
        bad = rows & ~zero & ~(xp.isfinite(nrm) & (nrm > 0) & xp.isfinite(br))
        nowhere = (zero & ~(br > 0)).any(-1)
        use = rows & ~zero & ~bad
        one = xp.ones_like(nrm)
        safe = xp.where(use, nrm, one)
        An = xp.where(use[:, :, None], A / safe[:, :, None], xp.zeros_like(A))
        bn = xp.where(use, br / safe, one)
        every = bad.any(-1) | ~use.any(-1)
    return An, bn, every, nowhere


def _locate_boxes(be, lb, ub, every, nowhere):
    """The boxes the grid is built from: (-inf, inf) where `every`, (inf, -inf) where `nowhere`; and the statistics that
    pick the axes, on the host (one read-back): st[0] / st[1] the extent of the finite boxes per axis, st[2] the sum of
    their widths, st[3] their number, st[4] the number of polytopes listed everywhere."""
    tor = be.torch
    xp = tor if tor is not None else np
    inf = float("inf")
    with np.errstate(all="ignore"):
        lb = xp.where(every[:, None], xp.full_like(lb, -inf), lb)
        ub = xp.where(every[:, None], xp.full_like(ub, inf), ub)
        lb = xp.where(nowhere[:, None], xp.full_like(lb, inf), lb)
        ub = xp.where(nowhere[:, None], xp.full_like(ub, -inf), ub)
        lb, ub = (lb.contiguous(), ub.contiguous()) if tor is not None else (np.ascontiguousarray(lb), np.ascontiguousarray(ub))
        fin = xp.isfinite(lb) & xp.isfinite(ub)
        zeros = xp.zeros_like(lb)
        amin, amax = (lambda t: t.amin(0), lambda t: t.amax(0)) if tor is not None else (lambda t: t.min(0), lambda t: t.max(0))
        f64 = (lambda t: t.to(tor.float64)) if tor is not None else (lambda t: t.astype(np.float64))
        st = xp.stack([amin(xp.where(fin, lb, xp.full_like(lb, inf))), amax(xp.where(fin, ub, xp.full_like(ub, -inf))),
                       xp.where(fin, ub - lb, zeros).sum(0), f64(fin.sum(0)), zeros[0] + f64((every & ~nowhere).sum())])
        st = st.cpu().numpy() if tor is not None else st
    return lb, ub, st


def _locate_desc(P, d, st):
    """The grid descriptor for the statistics of _locate_boxes -> (LocateGridDesc, axes) or (None, [])."""
    axes = _locate_axes(P, st[0], st[1], st[2], st[3], d)
    if not axes:
        return None, []
    desc = _lib.LocateGridDesc()
    desc.naxes = len(axes)
    for j, (k, lo, inv_h, res) in enumerate(axes):
        desc.axis[j], desc.lo[j], desc.inv_h[j], desc.res[j] = k, lo, inv_h, res
    for j in range(len(axes), 3):
        desc.res[j] = 1
    return desc, axes


def locate_grid(A, b, m=None, abs_tol=1e-7, max_items=_LOCATE_MAX_ITEMS, max_list=_LOCATE_MAX_LIST):
    """The culling grid of locate_batch for the packed table A[P, m_max, d], b[P, m_max], m[P] and this abs_tol.

    Every row is relaxed and normalised -- a_i / |a_i|, (b_i + abs_tol) / |a_i| -- and bbox_batch boxes the result; a
    polytope is listed in the cells its box (padded by 3.2e-9 of its largest coordinate, at least 1) reaches on up to three gridded axes.  A zero row
    with b_i + abs_tol > 0 is vacuous; a zero row otherwise means the polytope contains nothing (0 - b_i < abs_tol is
    false) and it is listed nowhere.  A polytope is listed in EVERY cell when its box is not to be had: bbox_batch status
    != 0, no rows, a row with inf / nan or a norm that under- or overflows.  Infinite sides span their axis.
    Declined -- kind "dense", nothing raised -- when the table has more than 64 rows per polytope (bbox_batch's limit;
    the dense kernel has none), when no axis separates the boxes, the lists would hold more than
    `max_items` entries or one of them more than `max_list`.
    numpy in: numpy lists; CUDA tensors in: resident tensors built on torch's current stream (two small read-backs: the
    box statistics that pick the axes, and the size of cell_items)."""
    be = _Backend(A)
    A, b, m, (P, m_max, d) = _packed(be, A, b, m)
    if d < 1 or d > MAX_D:
        raise _lib.UnsupportedSize("locate_grid: d=%d outside 1..%d" % (d, MAX_D))
    abs_tol = float(abs_tol)

    def dense(reason):
        return LocateGrid("dense", abs_tol, (P, m_max, d), reason=reason)
    if P == 0 or m_max == 0:
        return dense("no rows")
    if m_max > MAX_M:   # (the dense kernel, like contains_batch, has no row limit; the boxes have)
        return dense("m_max=%d: bbox_batch boxes polytopes of up to %d rows" % (m_max, MAX_M))
    An, bn, every, nowhere = _locate_rows(be, A, b, m, abs_tol)
    box = bbox_batch(An, bn, m)
    lb, ub, st = _locate_boxes(be, box["lb"], box["ub"], every | (box["status"] != 0), nowhere)
    if st[4, 0] > max_list:
        return dense("%d polytopes without a usable box: every list would exceed %d" % (int(st[4, 0]), max_list))
    desc, axes = _locate_desc(P, d, st)
    if desc is None:
        return dense("no axis along which the boxes are narrower than their common extent")
    G = int(np.prod([a[3] for a in axes]))
    hs = _HostStruct(desc)
    cell_start = be.out((G + 1,), np.int32, zero=True)
    max_len = be.out((1,), np.int32, zero=True)
    be.call("plp_locate_grid_count", P, d, lb, ub, _LOCATE_PAD, hs, cell_start, max_len, h2d=(lb, ub))
    if be.torch is not None:
        n_items, longest = (int(v) for v in be.torch.stack([cell_start[G], max_len[0]]).cpu())
    else:
        n_items, longest = int(cell_start[G]), int(max_len[0])
    if n_items > max_items or longest > max_list:
        return dense("%d list entries (budget %d), longest list %d (cap %d)" % (n_items, max_items, longest, max_list))
    cell_items = be.out((n_items,), np.int32, zero=True)
    cursor = be.out((G,), np.int32, zero=True)
    be.call("plp_locate_grid_fill", P, d, lb, ub, _LOCATE_PAD, hs, cell_start, cursor, cell_items, h2d=(lb, ub, cell_start))
    return LocateGrid("grid", abs_tol, (P, m_max, d), desc, cell_start, cell_items, n_items, longest)


def locate_batch(A, b, X, abs_tol=1e-7, m=None, count=False, grid="auto"):
    """For each of the N column vectors X[d, N] the index of the FIRST of the P packed polytopes that contains it, or -1
    (no counterpart in the reference; TuLiP's find_discrete_state loops `x in region`).

    -> first int32[N], or (first, count int32[N]) with count=True: how many polytopes contain the point.
    The dense answer is the definition: first[q] = min { p : all_{i < m[p]} (fl(A_p[i] . x_q) - b_p[i]) < abs_tol } in
    contains_batch's arithmetic, i.e. the arg-max over p of contains_batch(..., region=False) wherever a column holds a 1.
    A polytope with m[p] == 0 contains every point (NaN points too); a NaN coordinate is in no polytope that has a row.
    grid: None -- every polytope against every point; a LocateGrid from locate_grid (same table shape and abs_tol, else
    ValueError) -- candidates from the point's cell only; "auto" -- dense below 600 polytopes (the measured crossing at
    N = 2^20), else a grid built for this call.  A declined grid (kind "dense") runs the dense kernel."""
    be = _Backend(X)
    A, b, m, (P, m_max, d) = _packed(be, A, b, m)
    X = be.arr(X)
    if len(X.shape) != 2 or X.shape[0] != d:
        raise ValueError("points should be column vectors")
    N = int(X.shape[1])
    abs_tol = float(abs_tol)
    if isinstance(grid, LocateGrid):
        if grid.abs_tol != abs_tol or grid.shape != (P, m_max, d):
            raise ValueError("locate_batch: the LocateGrid was built for abs_tol=%r and a table of shape %s, not abs_tol=%r "
                             "and %s" % (grid.abs_tol, list(grid.shape), abs_tol, [P, m_max, d]))
        if grid.kind == "grid" and _is_torch(grid.cell_start) != (be.torch is not None):
            raise ValueError("locate_batch: the LocateGrid's lists and the points must both be numpy arrays or both CUDA tensors")
    elif grid is not None and not (isinstance(grid, str) and grid == "auto"):
        raise ValueError("grid must be 'auto', None or a LocateGrid")
    first = be.out((N,), np.int32, zero=True)
    cnt = be.out((N,), np.int32, zero=True) if count else None
    if N == 0:
        return (first, cnt) if count else first
    if isinstance(grid, str):
        grid = locate_grid(A, b, m, abs_tol) if P >= _LOCATE_AUTO_P else None
    if grid is not None and grid.kind == "grid":
        args = (_HostStruct(grid.desc), grid.cell_start, grid.cell_items if grid.n_items else None)
        h2d = (A, b, m, X, grid.cell_start, grid.cell_items)
    else:
        args, h2d = (None, None, None), (A, b, m, X)
    be.call("plp_locate", P, m_max, d, A, b, m, N, X, abs_tol, *args, first, cnt, h2d=h2d)
    return (first, cnt) if count else first


# flags of volume_batch (include/plp.h: PLP_VF_*)
VF_NONFINITE, VF_NOROWS = 1, 2
_VOLUME_MAX_N = 2 ** 31 - 1


def _volume_nsamples(d, nsamples=None):
    """The number of samples volume() draws in dimension d (ref :1565-1584): 50 / 500 / 3000 / 10000 by dimension unless
    `nsamples` is given; the reference's two ValueErrors for nsamples < 1 and for a non-integer."""
    N = {1: 50, 2: 500, 3: 3000}.get(d, 10000)
    if nsamples is not None and nsamples < 1:
        raise ValueError("`nsamples` must be >= 1, given:  {v}".format(v=nsamples))
    if nsamples is not None:
        N = nsamples
    if N != int(N):
        raise ValueError("it appears that a noninteger number of samples has been given, namely:  {v}".format(
            v=nsamples))
    return N


def _is_int(v):
    return isinstance(v, (int, np.integer)) and not isinstance(v, (bool, np.bool_))


def _volume_seeds(seed, B):
    """The seed of each polytope: None -> B spawned children of one fresh SeedSequence; an int -> that int B times (every
    polytope draws the same stream, as B calls of volume(P, seed=seed) do); B ints -> one each."""
    if seed is None:
        return list(np.random.SeedSequence().spawn(B))
    if _is_int(seed):
        if seed < 0:
            raise ValueError("`seed` must be a non-negative integer, given:  {v}".format(v=seed))
        return [int(seed)] * B
    if isinstance(seed, (str, bytes)) or not hasattr(seed, "__len__"):
        raise TypeError("`seed` must be None, an int or a sequence of B ints, got %s" % type(seed).__name__)
    seeds = list(seed)
    if len(seeds) != B:
        raise ValueError("`seed`: %d seeds for %d polytopes" % (len(seeds), B))
    for v in seeds:
        if not _is_int(v):
            raise TypeError("`seed` must be None, an int or a sequence of B ints, got an element of type %s"
                            % type(v).__name__)
        if v < 0:
            raise ValueError("`seed` must be a non-negative integer, given:  {v}".format(v=v))
    return [int(v) for v in seeds]


def _pcg64_words(seeds):
    """state[B, 2], inc[B, 2] (uint64, low word first) of np.random.PCG64(seed) -- what default_rng(seed) starts from."""
    B = len(seeds)
    words = np.empty((2, B, 2), np.uint64)
    memo = {}
    for k, sd in enumerate(seeds):
        key = sd if isinstance(sd, int) else id(sd)
        if key not in memo:
            st = np.random.PCG64(sd).state["state"]
            memo[key] = [(st[n] & 0xFFFFFFFFFFFFFFFF, st[n] >> 64) for n in ("state", "inc")]
        words[0, k], words[1, k] = memo[key]
    return words[0], words[1]


def volume_batch(A, b, m=None, nsamples=None, seed=None, lb=None, ub=None):
    """Monte-Carlo volume of B polytopes (volume, polytope.py:1529-1594): uniform samples in each polytope's bounding box,
    fraction strictly inside, times the volume of the box.  The samples are the ones the reference draws --
    np.random.default_rng(seed).random((d, N)), numpy's PCG64 stream -- generated on the device by jump-ahead, so no sample
    is uploaded and 4 bytes per polytope come back.
    `volume_batch(...)['volume'][k] == volume(P_k, nsamples, seed_k)` bit for bit on 'hip'.

    nsamples: None = the reference's table by dimension (50 / 500 / 3000 / 10000), else one N for the call.
    seed: None (every polytope a spawned child of one fresh np.random.SeedSequence), an int (every polytope draws the SAME
    stream, as B calls of volume(P, seed=seed) do) or B ints.
    lb, ub [B, d]: the bounding boxes; without them bbox_batch runs first and its device arrays are handed on.

    -> dict(volume[B], hits[B], nsamples, lb[B, d], ub[B, d], flags[B], seeds): numpy in, numpy out; torch CUDA tensors in,
    `hits` / `lb` / `ub` / `flags` are CUDA tensors and `volume` a CPU tensor (it is np.prod(ub - lb) * hits / N, the
    reference's expression, evaluated in numpy on the host: the call waits for the counts).  flags: VF_NONFINITE (a bound
    of the box is inf / nan, or bbox_batch did not handle the polytope: pass lb / ub) | VF_NOROWS (m = 0): not sampled,
    hits = 0 and volume = nan.  `seeds`: the seed of each polytope (what np.random.default_rng takes).
    d <= 16 and m_max <= 64 (UnsupportedSize beyond)."""
    be = _Backend(A)
    A, b, m, (B, m_max, d) = _packed(be, A, b, m)
    if d < 1:
        raise ValueError("A must be [B, m_max, d] with d >= 1")
    if (lb is None) != (ub is None):
        raise ValueError("lb and ub come together")
    for v in (lb, ub):
        if v is not None and tuple(v.shape) != (B, d):
            raise ValueError("lb / ub must be [B, d] = [%d, %d], got %s" % (B, d, tuple(v.shape)))
    N = _volume_nsamples(d, nsamples)
    if N > _VOLUME_MAX_N:
        raise ValueError("`nsamples` must be <= 2^31 - 1, given:  {v}".format(v=nsamples))
    N = int(N)
    seeds = _volume_seeds(seed, B)
    state, inc = _pcg64_words(seeds)
    torch = be.torch
    if lb is None:
        box = bbox_batch(A, b, m)
        ok = (box["status"] == 0)[:, None]
        if torch is not None:
            nan = torch.full((), float("nan"), dtype=torch.float64, device=A.device)
            lb, ub = torch.where(ok, box["lb"], nan), torch.where(ok, box["ub"], nan)
        else:
            lb, ub = np.where(ok, box["lb"], np.nan), np.where(ok, box["ub"], np.nan)
    if torch is not None:   # the boxes (when they came as numpy arrays) and the generator words go to the device here
        if not _is_torch(lb):
            lb, ub = _np(lb), _np(ub)
            _count_h2d(lb, ub)
            lb, ub = torch.as_tensor(lb).to(A.device), torch.as_tensor(ub).to(A.device)
        _count_h2d(state, inc)
        state, inc = torch.as_tensor(state.view(np.int64)).to(A.device), torch.as_tensor(inc.view(np.int64)).to(A.device)
    lb, ub = be.arr(lb), be.arr(ub)
    hits, flags = be.out((B,), np.uint32, zero=True), be.out((B,), np.int32, zero=True)
    be.call("plp_volume_hits", B, m_max, d, A, b, m, lb, ub, state, inc, N, hits, flags, h2d=(A, b, m, lb, ub, state, inc))
    if torch is not None:
        h_h, fl_h, lb_h, ub_h = hits.cpu().numpy(), flags.cpu().numpy(), lb.cpu().numpy(), ub.cpu().numpy()
    else:
        h_h, fl_h, lb_h, ub_h = hits, flags, lb, ub
    # the reference's expression (ref :1592), per polytope: np.prod(u_b - l_b) * aux / N
    with np.errstate(invalid="ignore"):
        vol = np.prod(ub_h - lb_h, axis=1) * h_h.astype(np.int64) / N
    vol[fl_h != 0] = np.nan
    if torch is not None:
        vol = torch.from_numpy(vol)
    return dict(volume=vol, hits=hits, nsamples=N, lb=lb, ub=ub, flags=flags, seeds=seeds)


# ------------------------------------------------------------------------------------- support functions
_SUPPORT_MAX_D = 4          # the shared-row kernel (csrc/plp_support.hip) walks in R^3 / R^4
_SUPPORT_CHUNK = 1 << 20    # LPs per lpsolve_batch call when rows are expanded per direction


def _support_input(be, a):
    """C / xc of support_batch on the backend of A (a numpy array beside CUDA tensors goes to their device)."""
    if be.torch is not None and not _is_torch(a):
        a = _np(a)
        _count_h2d(a)
        a = be.torch.as_tensor(a).to(be.device)
    return be.arr(a)


def _items_input(be, a, name, noun, B, d):
    """The per-polytope items of the shared-row calls (the directions C of support_batch, the points X of nearest_batch) on
    the backend of A: [K, d] shared by all polytopes or [B, K, d] -> (array, K, shared)."""
    a = _support_input(be, a)
    shp = tuple(a.shape)
    if len(shp) not in (2, 3):
        raise ValueError("%s must be [K, d] or [B, K, d], got %d dimensions" % (name, len(shp)))
    if shp[-1] != d or (len(shp) == 3 and shp[0] != B):
        raise ValueError("%s must be [K, %d] or [%d, K, %d], got %s" % (name, d, B, d, list(shp)))
    K = int(shp[-2])
    if K < 1:
        raise ValueError("%s holds no %s (K = 0)" % (name, noun))
    return a, K, len(shp) == 2


def _support_pairs(be, A, b, m, C, shared, pi, ji, flat, h, x, status):
    """The LPs (polytope pi[t], direction ji[t]) as generic LPs  min -c.x  s.t. A x <= b  through lpsolve_batch, the rows
    gathered per pair, at most _SUPPORT_CHUNK LPs per call; results written to position flat[t] of h / x / status."""
    hf, sf = h.reshape(-1), status.reshape(-1)
    xf = None if x is None else x.reshape(-1, x.shape[-1])
    for lo in range(0, int(pi.shape[0]), _SUPPORT_CHUNK):
        p, j, f = pi[lo:lo + _SUPPORT_CHUNK], ji[lo:lo + _SUPPORT_CHUNK], flat[lo:lo + _SUPPORT_CHUNK]
        c = -(C[j] if shared else C[p, j])
        sol = lpsolve_batch(c, A[p], b[p], None if m is None else m[p])
        st = sol["status"]
        sf[f] = st
        hv = -sol["fun"]
        hv[st == 3] = float("inf")
        hf[f] = hv
        if xf is not None:
            xf[f] = sol["x"]


def support_batch(A, b, C, m=None, xc=None, points=True, resolve=True):
    """Support functions  h_P(c) = max { c.x : A x <= b }  of B packed polytopes in K directions each: one LP per
    (polytope, direction), the rows of a polytope read once for all its directions (include/plp.h: plp_support_batch).

    A[B, m_max, d], b[B, m_max], m[B] as everywhere; C: the directions, [K, d] shared by all polytopes or [B, K, d].
    xc[B, d]: a strictly interior point per polytope; None: cheby_ball_batch runs first -- a polytope it finds infeasible
    gets status 2 in every direction, one without a usable centre (the Chebyshev LP not optimal, r <= 0, r = inf) a NaN
    centre, which the kernel hands back as status 1.
    -> dict(h[B, K], x[B, K, d] (None with points=False), status int32[B, K]); numpy in, numpy out; CUDA tensors in,
    tensors out on torch's current stream.
    status: 0 optimum; 3 unbounded in that direction (h = +inf, x = NaN); 2 the polytope is empty (h = x = NaN);
    4 numerical failure; 1 (only with resolve=False) not settled by the kernel.  resolve=True (the default) solves the
    pairs the kernel hands back through lpsolve_batch (c = -C, rows gathered per pair), so a caller sees lpsolve's codes
    only.  A zero direction gives h = 0, status 0 and x a feasible point.
    d <= 4 and m_max <= 64 run on the shared-row kernel.  Other shapes (d up to 16, any m_max lpsolve_batch takes) have no
    shared-row kernel yet: they go through lpsolve_batch with the rows expanded per direction, at most 2^20 LPs at a
    time, behind the same interface (xc is not used there).
    The kernel's status-0 answers pass two end checks: the final point against every row (1e-10 of the extent, and what
    it is outside a row by is worth at most 1e-10 of the extent in h), and an optimality certificate on the rows the walk
    ended on (multipliers >= 0, complementary slackness to 1e-10 and the cost's residual to 1e-12 of the extent).  So with E
    = max(1, |x|_inf, |h|): h <= h* + 1e-10 E, and h >= h* - 2e-10 E provided an optimal point lies within 100 max(1, |x - xc|)
    of x (for an optimal face reaching further the residual term is not bounded; plp_support.hpp).  What fails either
    check is handed back (status 1) and, with resolve=True, solved by lpsolve_batch under the verifier's certificate.  The
    kernel's own certificate is not that one."""
    be = _Backend(A)
    A, b, m, (B, m_max, d) = _packed(be, A, b, m)
    C, K, shared = _items_input(be, C, "C", "direction", B, d)
    if xc is not None:
        xc = _support_input(be, xc)
        if tuple(xc.shape) != (B, d):
            raise ValueError("xc must be [B, d] = [%d, %d], got %s" % (B, d, list(xc.shape)))
    xp = be.torch if be.torch is not None else np
    h, status = be.out((B, K), zero=True), be.out((B, K), np.int32, zero=True)
    x = be.out((B, K, d), zero=True) if points else None
    if B == 0:
        return dict(h=h, x=x, status=status)
    if d > _SUPPORT_MAX_D or m_max > MAX_M:   # no shared-row kernel at this shape yet
        n = B * K
        for lo in range(0, n, _SUPPORT_CHUNK):
            flat = xp.arange(lo, min(lo + _SUPPORT_CHUNK, n), **({} if be.torch is None else {"device": be.device}))
            _support_pairs(be, A, b, m, C, shared, flat // K, flat % K, flat, h, x, status)
        return dict(h=h, x=x, status=status)
    infeasible = None
    if xc is None:
        ball = cheby_ball_batch(A, b, m)
        r = ball["r"]
        ok = (ball["status"] == 0) & (r > 0) & (r < float("inf"))
        nan = float("nan") if be.torch is None else be.torch.full((), float("nan"), dtype=be.torch.float64, device=be.device)
        xc = xp.where(ok[:, None], ball["xc"], nan)
        infeasible = ball["status"] == 2
    be.call("plp_support_batch", B, m_max, d, A, b, m, K, C, 1 if shared else 0, xc, h, x, status, h2d=(A, b, m, C, xc))
    if infeasible is not None and bool(infeasible.any()):
        status[infeasible] = 2
        h[infeasible] = float("nan")
        if x is not None:
            x[infeasible] = float("nan")
    if resolve:
        pi, ji = xp.nonzero(status == 1) if be.torch is None else (status == 1).nonzero(as_tuple=True)
        if int(pi.shape[0]):
            _support_pairs(be, A, b, m, C, shared, pi, ji, pi * K + ji, h, x, status)
    return dict(h=h, x=x, status=status)


# ------------------------------------------------------------------------------------- nearest points
_NEAREST_MAX_D = 4           # the shared-row kernel (csrc/plp_nearest.hip) holds the active set of d <= 4 rows in registers
_NEAREST_END_TOL, _NEAREST_GAP_TOL, _NEAREST_RES_TOL = 1e-10, 1e-10, 1e-12   # the end checks of csrc/plp_nearest.hpp
_NEAREST_SUBSETS = 1 << 17   # row subsets per numpy call of the host routine


def _nearest_unit_rows(A, b):
    """Rows at unit 2-norm as the kernel stages them -> n, beta, |a| (a zero row: n = 0, beta = 0 for b >= 0, else -1)."""
    nrm = np.sqrt(np.sum(A * A, axis=1))
    z = nrm == 0
    s = np.where(z, 1.0, nrm)
    return A / s[:, None], np.where(z, np.where(b < 0, -1.0, 0.0), b / s), s


def _nearest_resolve_one(N, beta, p, xfeas=None):
    """The nearest point of { n_i.x <= beta_i } (unit rows) to p by enumeration: it is the orthogonal projection of p onto
    the affine hull of some face, so the closest FEASIBLE projection over all independent row subsets of size <= d is it.
    xfeas: a feasible point or None -- a row with beta_i - n_i.p above the distance of a known feasible point cannot be
    active and is left out first.  -> (dist, x, status, rows, lam): status 0 with both end checks of the kernel passed,
    4 when the best candidate fails them or an input is not finite, -1 when no subset gives a feasible point."""
    m, d = N.shape
    nanx = np.full(d, np.nan)
    none = np.zeros(0, np.int64)
    if not (np.all(np.isfinite(p)) and np.all(np.isfinite(N)) and np.all(np.isfinite(beta))):
        return np.nan, nanx, 4, none, np.zeros(0)
    live = np.nonzero((np.abs(N).sum(axis=1) > 0) | (beta < 0))[0]
    if np.any((np.abs(N[live]).sum(axis=1) == 0)):   # a zero row with b < 0
        return np.nan, nanx, -1, none, np.zeros(0)
    Nl, bl = N[live], beta[live]
    rows = live
    if xfeas is not None and np.all(np.isfinite(xfeas)) and live.size:
        s0 = bl - Nl @ xfeas
        if np.all(s0 >= 0):
            dr = p - xfeas
            ad = Nl @ dr
            t = min(1.0, float(np.min(s0[ad > 0] / ad[ad > 0], initial=1.0)))
            ub = float(np.linalg.norm(dr)) * (1.0 - t) * (1 + 1e-9) + 1e-12 * max(1.0, float(np.max(np.abs(p))))
            rows = live[(bl - Nl @ p) <= ub]
    pinf = max(1.0, float(np.max(np.abs(p), initial=0.0)))
    best = (np.inf, None, none, np.zeros(0))
    import itertools
    for s in range(0, min(d, rows.size) + 1):
        if s == 0:
            if np.max(Nl @ p - bl, initial=-np.inf) <= 0:
                return 0.0, p.copy(), 0, none, np.zeros(0)
            continue
        it = itertools.combinations(rows.tolist(), s)
        while True:
            S = np.array(list(itertools.islice(it, _NEAREST_SUBSETS)), dtype=np.int64).reshape(-1, s)
            if not S.shape[0]:
                break
            NS = N[S]
            G = NS @ NS.transpose(0, 2, 1)
            ok = np.linalg.det(G) > 1e-12
            if not ok.any():
                continue
            S, NS, G = S[ok], NS[ok], G[ok]
            c = np.linalg.solve(G, (NS @ p - beta[S])[:, :, None])[:, :, 0]
            x = p[None, :] - np.einsum("ns,nsk->nk", c, NS)
            E = np.maximum(pinf, np.abs(x).max(axis=1))
            viol = (x @ Nl.T - bl[None, :]).max(axis=1)
            dd = np.where(viol <= _NEAREST_END_TOL * E, np.linalg.norm(x - p[None, :], axis=1), np.inf)
            j = int(np.argmin(dd))
            if dd[j] < best[0]:
                best = (float(dd[j]), x[j], S[j], c[j])
    dist, x, S, lam = best
    if x is None:
        return np.nan, nanx, -1, none, np.zeros(0)
    # the kernel's two end checks on the candidate (feasibility held above)
    E = max(pinf, float(np.max(np.abs(x))))
    lam = np.maximum(lam, 0.0)
    gap = float(np.sum(lam * np.abs(beta[S] - N[S] @ x)))
    r = (p - x) - lam @ N[S]
    good = gap <= _NEAREST_GAP_TOL * E * max(dist, _NEAREST_GAP_TOL * E) and float(np.linalg.norm(r)) <= _NEAREST_RES_TOL * E
    if not good:
        return np.nan, nanx, 4, none, np.zeros(0)
    return dist, x, 0, S, lam


def _nearest_resolve(be, A, b, m, X, shared, out):
    """Raw status 1 settled on the host (nearest_batch: resolve=True), written into the arrays of `out`."""
    status = out["status"]
    host = (lambda a: a.cpu().numpy()) if be.torch is not None else (lambda a: a)
    pi, ji = np.nonzero(host(status) == 1)
    if not pi.size:
        return
    K, d = status.shape[1], A.shape[2]
    pu, inv = np.unique(pi, return_inverse=True)
    sel = pu if be.torch is None else be.torch.as_tensor(pu, device=be.device)
    Ah, bh = host(A[sel]), host(b[sel])
    mh = np.full(pu.size, A.shape[1]) if m is None else host(m[sel])
    ball = None
    n = pi.size
    res = dict(dist=np.full(n, np.nan), x=np.full((n, d), np.nan), status=np.full(n, 4, np.int32), face=np.zeros(n, np.uint64),
               lam=np.zeros((n, d)))
    Xh = host(X if shared else X[sel])
    units = {}
    for t in range(n):
        u = int(inv[t])
        mk = int(min(max(mh[u], 0), A.shape[1]))
        pt = Xh[ji[t]] if shared else Xh[u, ji[t]]
        if not (np.all(np.isfinite(pt)) and np.all(np.isfinite(Ah[u, :mk])) and np.all(np.isfinite(bh[u, :mk]))):
            continue   # status 4
        if ball is None:   # Chebyshev centres of the polytopes concerned: the cull's feasible point, and who is empty
            Af, bf = np.where(np.isfinite(Ah), Ah, 0.0), np.where(np.isfinite(bh), bh, 0.0)
            ball = cheby_ball_batch(Af, bf, np.ascontiguousarray(mh, dtype=np.int32))
        if u not in units:
            units[u] = _nearest_unit_rows(Ah[u, :mk], bh[u, :mk])
        N, beta, nrm = units[u]
        okc = ball["status"][u] == 0 and ball["r"][u] >= 0
        dd, xx, st, rows, lam = _nearest_resolve_one(N, beta, pt, ball["xc"][u] if okc else None)
        if st == -1:
            st = 2 if ball["status"][u] == 2 else 4
        res["status"][t] = st
        if st == 0:
            order = np.argsort(rows)
            res["dist"][t], res["x"][t] = dd, xx
            res["face"][t] = np.uint64(sum(1 << int(i) for i in rows))
            res["lam"][t, :rows.size] = (lam / nrm[rows])[order]
    flat = pi * K + ji
    for k, v in res.items():
        if out.get(k) is None:
            continue
        dst = out[k].reshape((-1,) + tuple(out[k].shape[2:]))
        if be.torch is not None:
            v = be.torch.as_tensor(v.view(np.int64) if v.dtype == np.uint64 else v).to(be.device)
            dst[be.torch.as_tensor(flat, device=be.device)] = v
        else:
            dst[flat] = v


def nearest_batch(A, b, X, m=None, points=True, faces=False, resolve=True):
    """Nearest points and Euclidean distances  min |x - p|_2  s.t.  A x <= b  of B packed polytopes to K points each: one
    strictly convex QP per (polytope, point), solved by a dual active-set walk per lane, the rows of a polytope read once
    for a whole chunk of its points (include/plp.h: plp_nearest_batch; csrc/plp_nearest.hpp).

    A[B, m_max, d], b[B, m_max], m[B] as everywhere; X: the points, [K, d] shared by all polytopes or [B, K, d].
    -> dict(dist[B, K], x[B, K, d] (None with points=False), face uint64[B, K] and lam[B, K, d] (None unless faces=True),
    status int32[B, K]); numpy in, numpy out; CUDA tensors in, tensors out on torch's current stream (face as int64: the
    same bits).  face: bit i set = row i is active at x; lam: the multipliers of those rows in ascending row order with
    respect to the rows as given, p - x = sum lam_j a_j, zero-padded.
    status: 0 optimum -- a point that violates no row comes back as x = p bit for bit with dist = 0; 2 the polytope is empty
    (dist = x = NaN); 4 numerical failure or an input that is not finite; 1 (only with resolve=False) not settled by the
    kernel.  Every status 0 passed, with E = max(1, |x|_inf, |p|_inf) and unit rows n_i: n_i.x - beta_i <= 1e-10 E on every row,
    and on the rows of face  sum lam_j |beta_j - n_j.x| <= 1e-10 E max(dist, 1e-10 E)  and  |(p - x) - sum lam_j n_j|_2 <= 1e-12 E,
    which bounds |x - x*| and dist - dist* (plp_nearest.hpp).  resolve=True (the default) settles what the kernel hands back
    on the host: the closest feasible projection onto a row subset of size <= d (rows that cannot be active culled by the
    Chebyshev centre's distance), under the same two checks or status 4; where no subset is feasible cheby_ball_batch decides
    between 2 and 4.  A caller with resolve=True never sees status 1.
    d <= 4 and m_max <= 64 only: other shapes raise UnsupportedSize.  There is NO fallback kernel for them."""
    be = _Backend(A)
    A, b, m, (B, m_max, d) = _packed(be, A, b, m)
    X, K, shared = _items_input(be, X, "X", "point", B, d)
    if d > _NEAREST_MAX_D or m_max > MAX_M:
        raise _lib.UnsupportedSize("nearest_batch: m_max=%d d=%d outside the shared-row kernel (m <= 64, d <= 4)" % (m_max, d))
    if B * K > 2 ** 31 - 1:
        raise _lib.UnsupportedSize("nearest_batch: B * K exceeds 2^31 - 1")
    out = dict(dist=be.out((B, K), zero=True), x=be.out((B, K, d), zero=True) if points else None,
               face=be.out((B, K), np.uint64, zero=True) if faces else None, lam=be.out((B, K, d), zero=True) if faces else None,
               status=be.out((B, K), np.int32, zero=True))
    if B == 0:
        return out
    be.call("plp_nearest_batch", B, m_max, d, A, b, m, K, X, 1 if shared else 0, out["dist"], out["x"], out["face"], out["lam"],
            out["status"], h2d=(A, b, m, X))
    if resolve:
        _nearest_resolve(be, A, b, m, X, shared, out)
    return out


def subset_batch(A, b, QA, Qb, m=None, mq=None, abs_tol=1e-7):
    """The exact H-in-H test  P_k <= Q_k  for B pairs: P_k = {A_k x <= b_k} lies in Q_k = {QA_k x <= Qb_k} iff the support
    function of P_k in the direction of every row of Q_k stays below that row's right-hand side.
    A[B, m_max, d], b[B, m_max], m[B];  QA[B, mq_max, d], Qb[B, mq_max], mq[B] (rows of Q_k in use) -> bool[B]:
    all(h_P(q_j) <= g_j + abs_tol) over the live rows (q_j, g_j) of Q -- support_batch with C = QA.  An empty P is a subset
    of anything; a direction in which P is unbounded means False.
    This is NOT what is_subset / `<=` of polytope_amd.polytope compute: those replay the reference's region_diff route (with
    its sampled volumes) and are not wired to this call."""
    be = _Backend(A)
    QA = _support_input(be, QA)
    if len(QA.shape) != 3:
        raise ValueError("QA must be [B, mq_max, d]")
    Bq, mq_max, _ = QA.shape
    Qb = _support_input(be, Qb).reshape(Bq, mq_max)
    res = support_batch(A, b, QA, m=m, points=False)
    h, st = res["h"], res["status"]
    xp = be.torch if be.torch is not None else np
    fine = ((st == 0) & (h <= Qb + abs_tol)) | (st == 2)
    if mq is not None:
        mq = _support_input(be, mq)
        rows = xp.arange(mq_max, **({} if be.torch is None else {"device": be.device}))
        fine = fine | (rows[None, :] >= mq.reshape(Bq, 1))
    return fine.all(1)


# ------------------------------------------------------------------------------------- vertex enumeration
# status codes of extreme_batch (include/plp.h: PLP_XS_*); the kernel sets the first three, this module the last two
XS_OK, XS_OVERFLOW, XS_EMPTY, XS_FLAT, XS_UNBOUNDED = 0, 1, 2, 3, 4
_EXTREME_MAX_D = 4   # the enumeration kernel (csrc/plp_extreme.hip)


def _extreme_vmax(d, n):
    """The most vertices a polytope of n facets has in dimension d (the upper-bound theorem), at least 1."""
    return max(1, {1: 2, 2: n, 3: 2 * n - 4}.get(d, n * (n - 3) // 2))


def _small_shape(name, what, A, b, m):
    """The shape checks of the enumeration calls (extreme_batch, volume_exact_batch, hull_batch) -> (B, rows_max, d).
    `what`: the words in which the messages of `name` differ -- (the array, its middle dimension, the count per member, what
    it does in dimension 1 .. 4, what it takes up to MAX_M of); b=None: there is no right-hand side to check."""
    arr, rows, cnt, does, items = what
    shape = lambda a: tuple(int(v) for v in (a.shape if hasattr(a, "shape") else np.shape(a)))   # noqa: E731
    shp = shape(A)
    if len(shp) != 3:
        raise ValueError("%s must be [B, %s, d], got %d dimensions" % (arr, rows, len(shp)))
    B, rows_max, d = shp
    if b is not None and shape(b) != (B, rows_max):
        raise ValueError("b must be [B, %s] = [%d, %d], got %s" % (rows, B, rows_max, list(shape(b))))
    if m is not None and int(np.prod(shape(m))) != B:
        raise ValueError("%s must be [B] = [%d]" % (cnt, B))
    if d < 1 or d > _EXTREME_MAX_D:
        raise ValueError("%s %s dimension 1 .. %d, got d = %d" % (name, does, _EXTREME_MAX_D, d))
    if rows_max > MAX_M:
        raise ValueError("%s takes %s, got %s = %d" % (name, items % MAX_M, rows, rows_max))
    return B, rows_max, d


def _extreme_unbounded(be, A, b, m, flat, d, box):
    """bool[B]: a side of the bounding box `box` = bbox_batch(A, b, m) is infinite (polytopes marked `flat` are not looked
    at).  bbox_batch answers from
    the Chebyshev centre; the polytopes it hands back (status 1: r < 1e-6, a Bland case) get the 2 d generic LPs, where
    an LP that ends unbounded -- or in any state but optimal / infeasible -- means the polytope is not vouched for.
    With CUDA tensors the host has to know whether anything was handed back: one flag is read back (a synchronisation),
    and the indices of those polytopes when there are any."""
    xp = be.torch if be.torch is not None else np
    inf = float("inf")
    open_ = ((box["lb"] == -inf) | (box["ub"] == inf) | (box["lb"] != box["lb"]) | (box["ub"] != box["ub"])).any(1)
    handled = box["status"] == 0
    unb = handled & open_ & ~flat
    back = ~handled & ~flat
    if bool(back.any()):
        rest = xp.nonzero(back)[0] if be.torch is None else back.nonzero(as_tuple=True)[0]
        nr = int(rest.shape[0])
        cost = np.vstack([np.eye(d), -np.eye(d)])
        if be.torch is not None:
            cost = be.torch.as_tensor(cost).to(be.device)
            rep = lambda a: a[rest].repeat_interleave(2 * d, dim=0)   # noqa: E731
            c = cost.repeat(nr, 1)
        else:
            rep = lambda a: np.repeat(a[rest], 2 * d, axis=0)   # noqa: E731
            c = np.tile(cost, (nr, 1))
        st = lpsolve_batch(c, rep(A), rep(b), None if m is None else rep(m))["status"].reshape(nr, 2 * d)
        unb[rest] = ((st != 0) & (st != 2)).any(1)
    return unb


def _reduced_and_bounded(be, A, b, m, abs_tol, d):
    """What reduce=True puts in front of an enumeration kernel, in this order on the device: reduce_batch, bbox_batch, the
    generic LPs for what bbox_batch handed back (_extreme_unbounded) -> (red, box, flat bool[B]: RF_EMPTY or r <= abs_tol,
    unb bool[B], keep: red["keep"], zero for a flat or unbounded member -- no live row: the kernel leaves at once)."""
    xp = be.torch if be.torch is not None else np
    red = reduce_batch(A, b, m, abs_tol=abs_tol)
    flat = ((red["flags"] & _lib.RF_EMPTY) != 0) | ~(red["r"] > abs_tol)
    box = bbox_batch(A, b, m)
    unb = _extreme_unbounded(be, A, b, m, flat, d, box)
    keep = xp.where(flat | unb, xp.zeros_like(red["keep"]), red["keep"])
    return red, box, flat, unb, keep


def _overlay(xp, flat, unb, x, if_flat, if_unb):
    """x[B] with if_flat where `flat`, else if_unb where `unb`."""
    return xp.where(flat, xp.full_like(x, if_flat), xp.where(unb, xp.full_like(x, if_unb), x))


def extreme_batch(A, b, m=None, v_max=None, reduce=True, abs_tol=1e-7, basis=False):
    """The vertices of B packed polytopes in one launch: for each polytope the vertices of reduce(P), each geometric vertex
    once (include/plp.h: plp_extreme_batch -- every d-subset of the rows solved and tested against all rows, one polytope
    per wavefront).  What extreme() computes per polytope (ref polytope.py:1597-1682), without its repeats of a degenerate
    vertex (one per simplex of the dual hull) and with a status where it returns None, raises or writes inf / nan.

    A[B, m_max, d], b[B, m_max], m[B] as everywhere; d <= 4 and m_max <= 64.
    -> dict(V[B, v_max, d] (NaN beyond count), count int32[B], status int32[B], basis int32[B, v_max, d] or None: the
    input rows of the subset that gave each vertex, -1 beyond count); numpy in, numpy out; CUDA tensors in, tensors out on
    torch's current stream.
    status: XS_OK all vertices written; XS_OVERFLOW more than v_max distinct vertices, the first v_max are written;
    XS_EMPTY no subset of the rows gives a feasible point; XS_FLAT empty or not full-dimensional (reduce_batch says
    RF_EMPTY, or r <= abs_tol); XS_UNBOUNDED a side of the bounding box is infinite.  FLAT and UNBOUNDED have count 0.
    reduce=True (the default): reduce_batch supplies the rows in use (`keep`), the radius and the flags, bbox_batch (and
    the generic LPs for what it hands back) decides boundedness, the kernel runs on what remains.  reduce=False: the
    kernel runs on the rows as given -- the caller vouches for boundedness and gets raw enumeration: rows that are redundant
    to 1e-7 but not identical do cross, and the crossings inside the polytope come back as vertices.
    v_max=None: sized from the upper-bound theorem for the largest number of rows in use in the batch (2, n, 2 n - 4,
    n (n - 3) / 2 for d = 1 .. 4; one scalar is read back for it).
    What waits for the device with CUDA tensors: that scalar (v_max=None), and with reduce=True one flag -- did bbox_batch
    hand a polytope back -- plus the indices of such polytopes when there are any.  reduce=False with v_max given
    enqueues the kernel and returns."""
    be = _Backend(A)
    B, m_max, d = _small_shape("extreme_batch", ("A", "m_max", "m", "enumerates bases in", "polytopes of up to %d rows"), A, b, m)
    if v_max is not None and (not _is_int(v_max) or v_max < 1):
        raise ValueError("`v_max` must be an integer >= 1, given:  {v}".format(v=v_max))
    A, b, m, _ = _packed(be, A, b, m)
    torch = be.torch
    xp = torch if torch is not None else np
    on = {} if torch is None else {"device": be.device}

    def empty_result(vm):
        return dict(V=be.out((B, vm, d), zero=True), count=be.out((B,), np.int32, zero=True),
                    status=be.out((B,), np.int32, zero=True), basis=be.out((B, vm, d), np.int32, zero=True) if basis else None)
    if B == 0:
        return empty_result(1 if v_max is None else int(v_max))
    keep = flat = unb = None
    if reduce:
        _, _, flat, unb, keep = _reduced_and_bounded(be, A, b, m, abs_tol, d)
    if v_max is None:
        if keep is not None:
            bits = xp.arange(64, **on) if torch is not None else np.arange(64, dtype=np.uint64)
            n = int((((keep[:, None] >> bits[None, :]) & 1) != 0).sum(1).max())
        elif m is not None:
            n = min(m_max, max(0, int(m.max())))
        else:
            n = m_max
        v_max = _extreme_vmax(d, n)
    v_max = int(v_max)
    res = empty_result(v_max)
    be.call("plp_extreme_batch", B, m_max, d, A, b, m, keep, v_max, res["V"], res["count"], res["basis"], res["status"],
            h2d=(A, b, m, keep))
    if reduce:
        res["status"] = _overlay(xp, flat, unb, res["status"], XS_FLAT, XS_UNBOUNDED)
    return res


# ------------------------------------------------------------------------------------- exact volume
# status codes of volume_exact_batch (include/plp.h: PLP_VS_*); the kernel sets the first three, this module VS_FLAT
VS_OK, VS_UNBOUNDED, VS_EMPTY, VS_FLAT = 0, 1, 2, 3


def volume_exact_batch(A, b, m=None, reduce=True, abs_tol=1e-7, areas=True):
    """The exact volumes and facet areas of B packed polytopes in one launch (include/plp.h: plp_vol_exact_batch --
    Lasserre's facet recursion on the rows, taken down to interval lengths; one polytope per wavefront).  Deterministic: no
    samples, no seed, the same bits from the same rows.  volume_batch stays the reference's Monte-Carlo estimate.

    A[B, m_max, d], b[B, m_max], m[B] as everywhere; d <= 4 and m_max <= 64.
    -> dict(volume[B], area[B, m_max] or None (areas=False): the (d-1)-measure of the facet of each input row, 0 for a row
    that is redundant, beyond m or a zero row (d = 1: 1 for the row at each end), status int32[B]); numpy in, numpy out; CUDA
    tensors in, tensors out on torch's current stream.
    status: VS_OK (a volume of 0 is a valid answer for an empty or flat set); VS_UNBOUNDED volume +inf; VS_EMPTY an
    infeasible zero row, volume 0; VS_FLAT empty or not full-dimensional (reduce_batch says RF_EMPTY, or r <= abs_tol):
    volume 0, areas 0.
    reduce=True (the default): reduce_batch supplies the rows in use (`keep`), the radius and the flags; bbox_batch (and the
    generic LPs for what it hands back) decides boundedness -- VS_UNBOUNDED, volume +inf, areas 0 -- and its box gives the
    kernel its reference point (the centre) and its unit of length (half the longest side), on which the rule's
    tolerances are absolute; a polytope bbox_batch handed back takes the Chebyshev centre and unit 1.
    reduce=False: the kernel runs on the rows as given, about the origin at unit 1.  It finds unbounded and empty members
    itself; rows closer than 1e-7 that reduce() would have merged each cut as they stand.
    The cost is n^(d-1) chains of n rows for n rows in use: (16, 3) costs about what extreme_batch does, (64, 4) runs for
    milliseconds per polytope.
    What waits for the device with CUDA tensors: with reduce=True one flag -- did bbox_batch hand a polytope back -- plus
    the indices of such polytopes when there are any.  reduce=False enqueues the kernel and returns."""
    be = _Backend(A)
    B, m_max, d = _small_shape("volume_exact_batch", ("A", "m_max", "m", "takes", "polytopes of up to %d rows"), A, b, m)
    A, b, m, _ = _packed(be, A, b, m)
    xp = be.torch if be.torch is not None else np
    res = dict(volume=be.out((B,), zero=True), area=be.out((B, m_max), zero=True) if areas else None,
               status=be.out((B,), np.int32, zero=True))
    if B == 0:
        return res
    keep = xc = scale = flat = unb = None
    if reduce:
        red, box, flat, unb, keep = _reduced_and_bounded(be, A, b, m, abs_tol, d)
        with np.errstate(invalid="ignore"):   # (an open box: inf - inf, masked below)
            side, mid = box["ub"] - box["lb"], 0.5 * (box["lb"] + box["ub"])
        boxed = (box["status"] == 0) & ~flat & ~unb & (side == side).all(1) & (side > 0).all(1)
        xc = xp.where(boxed[:, None], mid, red["xc"])
        xc = xp.where((xc == xc) & ~(flat | unb)[:, None], xc, xp.zeros_like(xc))
        scale = xp.where(boxed, 0.5 * side.max(1)[0] if be.torch is not None else 0.5 * side.max(1), xp.ones_like(red["r"]))
        xc, scale = be.arr(xc), be.arr(scale)
    be.call("plp_vol_exact_batch", B, m_max, d, A, b, m, keep, xc, scale, res["volume"], res["area"], res["status"],
            h2d=(A, b, m, keep, xc, scale))
    if reduce:
        res["status"] = _overlay(xp, flat, unb, res["status"], VS_FLAT, VS_UNBOUNDED)
        res["volume"] = _overlay(xp, flat, unb, res["volume"], 0.0, float("inf"))
        if areas:
            res["area"] = xp.where((flat | unb)[:, None], xp.zeros_like(res["area"]), res["area"])
    return res


# ------------------------------------------------------------------------------------- facet enumeration
# status codes of hull_batch (include/plp.h: PLP_HS_*)
HS_OK, HS_OVERFLOW, HS_FLAT = 0, 1, 2


def hull_batch(X, n=None, f_max=None, basis=False):
    """The facets of B packed point sets in one launch: rows A x <= b of the convex hull of each set, each face once
    (include/plp.h: plp_hull_batch -- every d-subset of the points spans a hyperplane, which is a facet when all points lie
    on one side of it; one point set per wavefront).  What quickhull() computes per set (ref quickhull.py:141-359), without
    its repeats of a face that carries more than d points and with a status where it prints "not fully dimensional".

    X[B, n_max, d], n[B] (the points in use per set, None = n_max); d <= 4 and n_max <= 64.
    -> dict(A[B, f_max, d] unit normals and b[B, f_max] (NaN beyond count), on uint64[B, f_max]: bit i set when point i
    lies on the facet (0 beyond count), count int32[B], status int32[B], basis int32[B, f_max, d] or None: the points of
    the subset that gave each facet, -1 beyond count); numpy in, numpy out; CUDA tensors in, tensors out on torch's current
    stream, `on` then as int64 with the same bits (torch has no unsigned words).  numpy input is checked for inf / nan by
    the library, padding included: the V of extreme_batch carries NaN beyond count, so pass it on as CUDA tensors or zero it.
    The rule: the points are moved to the centre of their bounding box and scaled to [-1, 1]^d, so the tolerances are
    absolute; a subset is skipped when its normal is shorter than 1e-12 of the product of its edge lengths; a point is on
    a plane, or on its right side, to 1e-9; all points on one plane means the set is flat; a facet is dropped when one
    accepted before it has the same unit normal and offset to 1e-9.
    status: HS_OK all facets written; HS_OVERFLOW more than f_max distinct facets, the first f_max are written; HS_FLAT
    fewer than d + 1 points, or all of them in one hyperplane: count 0.
    f_max=None: sized from the upper-bound theorem for the largest n of the batch (2, n, 2 n - 4, n (n - 3) / 2 for
    d = 1 .. 4, the bound of extreme_batch by duality; one scalar is read back for it when n is a CUDA tensor).  With
    f_max given the call enqueues the kernel and returns.
    Not provided: a vertex list -- the bits of `on` name the points on the boundary, and extreme_batch on the rows gives the
    vertices.  The rows are neither reduced (a near-degenerate subset can repeat a face as a second, slightly tilted row)
    nor passed through Polytope."""
    be = _Backend(X)
    B, n_max, d = _small_shape("hull_batch", ("X", "n_max", "n", "enumerates hyperplanes in", "point sets of up to %d points"),
                               X, None, n)
    if f_max is not None and (not _is_int(f_max) or f_max < 1):
        raise ValueError("`f_max` must be an integer >= 1, given:  {v}".format(v=f_max))
    X, n = be.arr(X), be.arr(n, np.int32, (B,))
    if f_max is None:
        f_max = _extreme_vmax(d, n_max if n is None or B == 0 else min(n_max, max(0, int(n.max()))))
    f_max = int(f_max)
    res = dict(A=be.out((B, f_max, d), zero=True), b=be.out((B, f_max), zero=True), on=be.out((B, f_max), np.uint64, zero=True),
               count=be.out((B,), np.int32, zero=True), status=be.out((B,), np.int32, zero=True),
               basis=be.out((B, f_max, d), np.int32, zero=True) if basis else None)
    if B:
        be.call("plp_hull_batch", B, n_max, d, X, n, None, f_max, res["A"], res["b"], res["on"], res["count"], res["basis"],
                res["status"], h2d=(X, n))
    return res


def assign_batch(X, normals, offsets, abs_tol=1e-7):
    """quickhull outside-set assignment + furthest point (quickhull.py:87-102,117-121,224-245).

    X[N, d] points (rows), normals[F, d], offsets[F]
    -> dict(facet int32[N] (-1 inside), dist[N], argmax int64[F] (-1 none), maxd[F])
    """
    be = _Backend(X)
    X = be.arr(X)
    N, d = X.shape
    normals = be.arr(normals, shape=(-1, d))
    F = normals.shape[0]
    offsets = be.arr(offsets, shape=(F,))
    fop, dist = be.out((N,), np.int32), be.out((N,))
    am, mx = be.out((F,), np.int64), be.out((F,))
    be.call("plp_assign", N, d, X, F, normals, offsets, float(abs_tol), fop, dist, am, mx, h2d=(X, normals, offsets))
    return dict(facet=fop, dist=dist, argmax=am, maxd=mx)


class HullSession:
    """Outside sets of one quickhull run, resident on the device (include/plp.h: plp_hull_*).

    The N points are uploaded once; per iteration `reassign` moves the points owned by the dead
    (visible) facets to the new facets and returns, per new facet, how many points it received and
    which one is furthest (quickhull.py:273-283, :311-336, :87-102).
    """

    def __init__(self, X):
        lib = _lib.load()
        X = _np(X)
        if X.ndim != 2:
            raise ValueError("points must be an (N, d) array")
        _finite_or_raise("HullSession", X)
        self.N, self.d = X.shape
        self._ctx = _lib.context()
        h = C.c_void_p()
        _lib.check(lib.plp_hull_create(self._ctx.handle, self.N, self.d, _ptr(X), C.byref(h)), "plp_hull_create")
        self._h = h

    def drop(self, idx):
        idx = np.ascontiguousarray(idx, dtype=np.int64).ravel()
        _lib.check(_lib.load().plp_hull_drop(self._h, idx.size, _ptr(idx)), "plp_hull_drop")

    def reassign(self, dead_ids, normals, offsets, abs_tol=1e-7):
        """-> (new_id0, count int64[n_new], argmax int64[n_new] (-1 none), maxd[n_new])"""
        dead = np.ascontiguousarray(dead_ids, dtype=np.int32).ravel()
        normals = _np(normals).reshape(-1, self.d)
        n_new = normals.shape[0]
        offsets = _np(offsets).reshape(n_new)
        am = np.empty(n_new, np.int64)
        mx = np.empty(n_new)
        cnt = np.empty(n_new, np.int64)
        id0 = C.c_int32(0)
        _lib.check(_lib.load().plp_hull_reassign(self._h, dead.size, _ptr(dead), n_new, _ptr(normals), _ptr(offsets),
                                                 float(abs_tol), C.byref(id0), _ptr(am), _ptr(mx), _ptr(cnt)),
                   "plp_hull_reassign")
        return int(id0.value), cnt, am, mx

    def read(self):
        """-> (owner int32[N], dist[N]) copied to the host"""
        owner = np.empty(self.N, np.int32)
        dist = np.empty(self.N)
        _lib.check(_lib.load().plp_hull_read(self._h, _ptr(owner), _ptr(dist)), "plp_hull_read")
        return owner, dist

    def close(self):
        if getattr(self, "_h", None):
            _lib.load().plp_hull_destroy(self._h)
            self._h = None

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass


def hull_reassign_dev(X, owner, dist, dead, new_id0, normals, offsets, abs_tol=1e-7):
    """Stateless form on torch CUDA tensors (updates owner/dist in place) -> dict(count, argmax, maxd)."""
    lib = _lib.load()
    torch, ctx, stream = _torch_stream_ctx(X)
    N, d = X.shape
    n_new = normals.shape[0]
    am = torch.empty((n_new,), dtype=torch.int64, device=X.device)
    mx = torch.empty((n_new,), dtype=torch.float64, device=X.device)
    cnt = torch.empty((n_new,), dtype=torch.int64, device=X.device)
    _lib.check(lib.plp_hull_reassign_dev(ctx.handle, stream, N, d, _ptr(X), _ptr(owner), _ptr(dist), _ptr(dead),
                                         int(new_id0), n_new, _ptr(normals), _ptr(offsets), float(abs_tol),
                                         _ptr(am), _ptr(mx), _ptr(cnt)), "plp_hull_reassign_dev")
    return dict(count=cnt, argmax=am, maxd=mx)


def _cells(what, A, b, m):
    """The table of the pair operations: cells A[n, m_max, d], b[n, m_max], m -> (backend, A, b, m, n, m_max, d); numpy
    inputs are checked for inf / nan here."""
    be = _Backend(A)
    A, b, m, (n, m_max, d) = _packed(be, A, b, m)
    if be.torch is None:
        _finite_or_raise(what, A, b)
    return be, A, b, m, n, m_max, d


def adjacent_pairs(A, b, m=None, abs_tol=1e-7):
    """Adjacency matrix of n single-polytope cells (prop2partition.py:46-63 over polytope.py:1843-1866):
    uint8[n, n], symmetric, ones on the diagonal.  A[n, m_max, d], b[n, m_max]; 2*m_max <= 64, d <= 16.
    The n(n-1)/2 stacked, abs_tol-inflated pair LPs are formed on the device."""
    be, A, b, m, n, m_max, d = _cells("adjacent_pairs", A, b, m)
    adj = be.out((n, n), np.uint8, zero=True)
    be.call("plp_adjacent_pairs", n, m_max, d, A, b, m, float(abs_tol), adj, h2d=(A, b, m))
    return adj


def overlap_pairs(A, b, m=None, abs_tol=1e-7):
    """uint8[n, n]: 1 where the intersection of cells i and j is full-dimensional (Chebyshev radius of the
    stacked rows > abs_tol) -- the pair test of Partition.are_disjoint (prop2partition.py:146-149); ones
    on the diagonal.  A[n, m_max, d], b[n, m_max]; 2*m_max <= 64, d <= 16."""
    be, A, b, m, n, m_max, d = _cells("overlap_pairs", A, b, m)
    out = be.out((n, n), np.uint8, zero=True)
    be.call("plp_overlap_pairs", n, m_max, d, A, b, m, float(abs_tol), out, h2d=(A, b, m))
    return out


def overlap_cross(A, b, n1, m=None, thresh=1e-7):
    """uint8[n1, n - n1]: 1 where the stack [cell a; cell c] of cell a < n1 of the table and cell c >= n1 has a Chebyshev
    radius > thresh -- the opening scan of region_diff (polytope.py:2148-2158) for every (minuend member, subtrahend
    cell) pair at once.  A[n, m_max, d], b[n, m_max]; 2 * m_max <= 64, d <= 16."""
    n1 = int(n1)
    be, A, b, m, n, m_max, d = _cells("overlap_cross", A, b, m)
    out = be.out((n1, n - n1), np.uint8, zero=True)
    be.call("plp_overlap_cross", n1, n - n1, m_max, d, A, b, m, float(thresh), out, h2d=(A, b, m))
    return out


def adjacent_pairs_range(A, b, pair_lo, pair_hi, m=None, abs_tol=1e-7):
    """Adjacency of the cell pairs pair_lo <= p < pair_hi (p = i (i - 1) / 2 + j, j < i) -> uint8[pair_hi - pair_lo];
    one rank's shard of the O(n^2) loop of find_adjacent_regions (prop2partition.py:57-61)."""
    lo, hi = int(pair_lo), int(pair_hi)
    be, A, b, m, n, m_max, d = _cells("adjacent_pairs_range", A, b, m)
    out = be.out((max(hi - lo, 0),), np.uint8, zero=True)
    be.call("plp_adjacent_pairs_range", n, m_max, d, A, b, m, float(abs_tol), lo, hi, out, h2d=(A, b, m))
    return out


# ------------------------------------------------------------------------------------- sparse pair screens
# box_pairs(grid="auto"): every partner box-tested below this many cells, a grid built above.  NOT MEASURED:
# at 1024 cells the brute walk of a cell is at most 16 steps of 64 partners, about what a walk over a 2 x 2 x 2 cell range
# costs; which of the two runs changes the time only, never the set.
_BOX_PAIRS_AUTO_N = 1024
PAIR_BAD = 255    # include/plp.h: PLP_PAIR_BAD


class _BoxPairs(object):
    """The broad phase of one table of boxes: the grid (or none), per_cell int64[n + 1] and K = per_cell[n] after the count
    pass; fill(cell_lo, cell_hi) then gives the candidate pairs of whole cells."""

    def __init__(self, be, lb, ub, n1, pad, grid):
        self.be = be
        lb, ub = be.arr(lb), be.arr(ub)
        if len(lb.shape) != 2 or tuple(ub.shape) != tuple(lb.shape):
            raise ValueError("box_pairs: lb and ub must both be [n, d]")
        self.n, self.d = int(lb.shape[0]), int(lb.shape[1])
        self.n1 = 0 if n1 is None else int(n1)
        if n1 is not None and not (0 < self.n1 <= self.n):
            raise ValueError("box_pairs: n1 must lie in 1..n (the cells of the first list)")
        if self.d < 1 or self.d > MAX_D:
            raise _lib.UnsupportedSize("box_pairs: d=%d outside 1..%d" % (self.d, MAX_D))
        if not (isinstance(grid, str) and grid in ("auto", "grid")) and grid is not None:
            raise ValueError("grid must be 'auto', 'grid' or None")
        self.pad = float(pad)
        self.lb, self.ub = lb, ub
        self.lists, self.desc, self.reason = (None, None, None), None, "not asked for"
        if grid == "grid" or (grid == "auto" and self.n >= _BOX_PAIRS_AUTO_N):
            self._build_grid()
        self.per_cell = be.out((self.n + 1,), np.int64, zero=True)
        be.call("plp_box_pairs_count", self.n, self.d, self.lb, self.ub, self.pad, *self.lists, self.n1, self.per_cell,
                h2d=(self.lb, self.ub) + tuple(a for a in self.lists[1:] if a is not None))
        self.K = int(self.per_cell[self.n])   # (resident: the one read-back of the count pass)
        self._pc_host = None

    def _build_grid(self):
        """The cell lists of the point-location grid over these boxes (locate_grid's passes); declined -- self.lists stays
        (None, None, None) and the kernels box-test every partner -- as locate_grid declines."""
        be, n, d = self.be, self.n, self.d
        xp = be.torch if be.torch is not None else np
        if n == 0:
            self.reason = "no cells"
            return
        never = xp.zeros_like(self.lb[:, 0]) != 0
        self.lb, self.ub, st = _locate_boxes(be, self.lb, self.ub, never, never)
        desc, axes = _locate_desc(n, d, st)
        if desc is None:
            self.reason = "no axis along which the boxes are narrower than their common extent"
            return
        G = int(np.prod([a[3] for a in axes]))
        hs = _HostStruct(desc)
        cell_start = be.out((G + 1,), np.int32, zero=True)
        max_len = be.out((1,), np.int32, zero=True)
        be.call("plp_locate_grid_count", n, d, self.lb, self.ub, self.pad, hs, cell_start, max_len, h2d=(self.lb, self.ub))
        if be.torch is not None:
            n_items, longest = (int(v) for v in be.torch.stack([cell_start[G], max_len[0]]).cpu())
        else:
            n_items, longest = int(cell_start[G]), int(max_len[0])
        if n_items > _LOCATE_MAX_ITEMS or longest > _LOCATE_MAX_LIST:
            self.reason = "%d list entries (budget %d), longest list %d (cap %d)" % (n_items, _LOCATE_MAX_ITEMS, longest,
                                                                                    _LOCATE_MAX_LIST)
            return
        cell_items = be.out((max(n_items, 1),), np.int32, zero=True)
        cursor = be.out((G,), np.int32, zero=True)
        be.call("plp_locate_grid_fill", n, d, self.lb, self.ub, self.pad, hs, cell_start, cursor, cell_items,
                h2d=(self.lb, self.ub, cell_start))
        self.lists, self.reason, self.desc = (hs, cell_start, cell_items), "", desc

    def fill(self, cell_lo=0, cell_hi=None):
        """int32[K', 2]: the candidate pairs of the cells cell_lo <= i < cell_hi, sorted by (i, j)."""
        cell_hi = self.n if cell_hi is None else int(cell_hi)
        if cell_lo == 0 and cell_hi == self.n:
            k = self.K
        else:
            k = int(self.per_cell[cell_hi]) - int(self.per_cell[cell_lo]) if self._pc_host is None else \
                int(self._pc_host[cell_hi] - self._pc_host[cell_lo])
        pairs = self.be.out((k, 2), np.int32, zero=True)
        if k:
            self.be.call("plp_box_pairs_fill", self.n, self.d, self.lb, self.ub, self.pad, *self.lists, self.n1, self.per_cell,
                         int(cell_lo), cell_hi, pairs, h2d=(self.lb, self.ub, self.per_cell))
        return pairs

    def chunks(self, max_candidates):
        """[(cell_lo, cell_hi)]: whole cells, at most max_candidates pairs each (a single cell with more is a chunk of its
        own); one chunk, and no read-back of per_cell, when everything fits."""
        if self.K <= max_candidates:
            return [(0, self.n)] if self.K else []
        pc = self.per_cell.cpu().numpy() if self.be.torch is not None else self.per_cell
        self._pc_host = pc
        out, lo = [], 0
        while lo < self.n and pc[lo] < pc[self.n]:
            hi = int(np.searchsorted(pc, pc[lo] + max_candidates, side="right")) - 1
            hi = min(max(hi, lo + 1), self.n)
            if pc[hi] > pc[lo]:
                out.append((lo, hi))
            lo = hi
        return out


def box_pairs(lb, ub, n1=None, pad=_LOCATE_PAD, grid="auto"):
    """The pairs of n boxes lb[n, d], ub[n, d] that meet -- the broad phase of the sparse pair calls.

    Box p is padded to [lb_p - pad', ub_p + pad'], pad' = pad * max(1, its largest finite |bound|); NaN bounds and infinite
    sides span their axis.  (i, j), j < i, is a candidate iff the padded boxes meet on all d axes; with n1 the table holds
    two lists, n1 boxes and then n - n1, and the candidates are the (a, c) with a < n1 <= c.
    -> dict(pairs int32[K, 2] sorted by (i, j), per_cell int64[n + 1] (cell i's partners are pairs[per_cell[i] :
    per_cell[i + 1]]), ncand = K, grid = the LocateGridDesc used or None).
    grid: None -- every partner is box-tested; "grid" -- partners are met through the cell lists of the point-location grid
    (locate_grid's passes over these boxes), each pair in one canonical cell; "auto" -- the grid from 1024 boxes on.  The
    set is the same, integer for integer; a declined grid (no separating axis, lists over budget) runs the first form.
    numpy in: numpy out; CUDA tensors in: resident tensors on torch's current stream (read-backs: K, and the grid's sizes)."""
    bp = _BoxPairs(_Backend(lb), lb, ub, n1, pad, grid)
    return dict(pairs=bp.fill(), per_cell=bp.per_cell, ncand=bp.K, grid=bp.desc)


def pair_verdicts(A, b, pairs, m=None, inflate=0.0, thresh=1e-7):
    """uint8[K]: for each listed pair (pairs[t, 0], pairs[t, 1]) of the n cells A[n, m_max, d], b[n, m_max] the verdict of
    the dense pair calls -- 1 iff the stack of the two cells, every b raised by `inflate`, has a Chebyshev radius > thresh
    (adjacent_pairs: inflate = abs_tol, thresh = abs_tol / 10; overlap_pairs / overlap_cross: inflate = 0, thresh =
    abs_tol), through the same engines and careful pass.  pairs int32[K, 2]; a pair may appear more than once, in either
    order.  2 * m_max <= 64, d <= 16.  numpy: an index outside [0, n) or a pair (i, i) raises PlpError; CUDA tensors
    (nothing synchronises, so the list is not read by the host): such a pair gets 255 and nothing is read for it."""
    be, A, b, m, n, m_max, d = _cells("pair_verdicts", A, b, m)
    pairs = be.arr(pairs, np.int32)
    if len(pairs.shape) != 2 or pairs.shape[1] != 2:
        raise ValueError("pairs must be [K, 2]")
    K = int(pairs.shape[0])
    out = be.out((K,), np.uint8, zero=True)
    be.call("plp_pair_list", n, m_max, d, A, b, m, float(inflate), float(thresh), K, pairs, out, h2d=(A, b, m, pairs))
    return out


def _outer_boxes(be, A, b, m, inflate):
    """Outer boxes of the cells {A x <= b + inflate}: bbox_batch's, and every side infinite for a cell whose box is not to
    be had -- status != 0, a zero row, a non-finite entry, no rows.  (Never "nowhere": only outer boxes are safe.)"""
    tor = be.torch
    xp = tor if tor is not None else np
    kw = {} if tor is None else {"device": be.device}
    n, m_max = int(A.shape[0]), int(A.shape[1])
    inf = float("inf")
    with np.errstate(all="ignore"):
        br = b + inflate
        box = bbox_batch(A, br, m)
        rows = (xp.arange(m_max, **kw)[None, :] < m[:, None]) if m is not None else \
            xp.ones((n, m_max), dtype=(bool if tor is None else tor.bool), **kw)
        zero = rows & (A == 0).all(-1)
        bad = rows & ~(xp.isfinite(A).all(-1) & xp.isfinite(br))
        every = (box["status"] != 0) | zero.any(-1) | bad.any(-1) | ~rows.any(-1)
        lb = xp.where(every[:, None], xp.full_like(box["lb"], -inf), box["lb"])
        ub = xp.where(every[:, None], xp.full_like(box["ub"], inf), box["ub"])
    return lb, ub


def _pairs_sparse(what, A, b, m, inflate, thresh, n1, boxes, max_candidates, grid="auto"):
    """Broad phase, then per chunk of whole cells: fill -> listed pair LPs -> the positives -> dict(pairs, ncand)."""
    be, A, b, m, n, m_max, d = _cells(what, A, b, m)
    if m_max < 1 or 2 * m_max > MAX_M or d < 1 or d > MAX_D:
        raise _lib.UnsupportedSize("%s: m_max=%d d=%d outside envelope (2*m_max<=64, d<=16)" % (what, m_max, d))
    max_candidates = int(max_candidates)
    if max_candidates < 1:
        raise ValueError("%s: max_candidates must be at least 1" % what)
    if boxes is None:
        lb, ub = _outer_boxes(be, A, b, m, float(inflate)) if n else (be.out((0, d)), be.out((0, d)))
    else:
        lb, ub = boxes
        if tuple(lb.shape) != (n, d) or tuple(ub.shape) != (n, d):
            raise ValueError("%s: boxes must be (lb[n, d], ub[n, d])" % what)
    bp = _BoxPairs(be, lb, ub, n1, _LOCATE_PAD, grid)
    found = []
    for lo, hi in bp.chunks(max_candidates):
        cand = bp.fill(lo, hi)
        K = int(cand.shape[0])
        v = be.out((K,), np.uint8, zero=True)
        be.call("plp_pair_list", n, m_max, d, A, b, m, float(inflate), float(thresh), K, cand, v, h2d=(A, b, m, cand))
        found.append(cand[v != 0])
    if not found:
        pairs = be.out((0, 2), np.int32, zero=True)
    elif len(found) == 1:
        pairs = found[0]
    else:
        pairs = be.torch.cat(found) if be.torch is not None else np.concatenate(found)
    return dict(pairs=pairs, ncand=bp.K)


def adjacent_pairs_sparse(A, b, m=None, abs_tol=1e-7, boxes=None, max_candidates=1 << 24):
    """The adjacent pairs of n single-polytope cells as a list: dict(pairs int32[K, 2], ncand) with pairs EXACTLY the
    nonzeros of tril(adjacent_pairs(A, b, m, abs_tol), -1) -- (i, j), i > j, sorted by (i, j) -- and ncand the number of
    pair LPs solved.  A[n, m_max, d], b[n, m_max]; 2 * m_max <= 64, d <= 16; no n x n matrix is formed.

    Only pairs whose outer boxes meet are solved (box_pairs): a pair counts iff the stack of the two abs_tol-inflated cells
    holds a ball of radius > abs_tol / 10, and that ball lies in both boxes.  boxes: None -- bbox_batch(A, b + abs_tol, m),
    every side infinite for a cell without a usable box (box status != 0, a zero row, a non-finite entry, no rows); or
    (lb[n, d], ub[n, d]), which MUST be outer boxes of the inflated cells {A_p x <= b_p + abs_tol} -- a side that cuts
    into a cell loses pairs silently.  The candidates go through the pair LPs in chunks of whole cells of at most
    max_candidates pairs (8 bytes of indices and one of verdict each; a cell with more partners is a chunk of its own).
    numpy in: numpy out; CUDA tensors in: resident tensors on torch's current stream."""
    abs_tol = float(abs_tol)
    return _pairs_sparse("adjacent_pairs_sparse", A, b, m, abs_tol, abs_tol / 10, None, boxes, max_candidates)


def overlap_pairs_sparse(A, b, m=None, abs_tol=1e-7, boxes=None, max_candidates=1 << 24):
    """As adjacent_pairs_sparse for overlap: pairs = the nonzeros of tril(overlap_pairs(A, b, m, abs_tol), -1); nothing is
    inflated (boxes passed in are outer boxes of the cells themselves) and a pair counts iff the stack holds a ball of
    radius > abs_tol."""
    return _pairs_sparse("overlap_pairs_sparse", A, b, m, 0.0, float(abs_tol), None, boxes, max_candidates)


def overlap_cross_sparse(A, b, n1, m=None, thresh=1e-7, boxes=None, max_candidates=1 << 24):
    """As overlap_pairs_sparse for two lists in one table (overlap_cross): pairs = the nonzeros (a, c) of
    overlap_cross(A, b, n1, m, thresh), a < n1 a cell of the first list and c < n - n1 one of the second, sorted by (a, c)."""
    n1 = int(n1)
    if n1 == 0:   # (an empty first list, as overlap_cross; the library reads n1 = 0 as "all pairs")
        be = _Backend(A)
        return dict(pairs=be.out((0, 2), np.int32, zero=True), ncand=0)
    res = _pairs_sparse("overlap_cross_sparse", A, b, m, 0.0, float(thresh), n1, boxes, max_candidates)
    if int(res["pairs"].shape[0]):
        res["pairs"][:, 1] -= n1
    return res


# ------------------------------------------------------------------------------------- intersections of listed pairs
RF_EMPTY, RF_LPFAIL, RF_F1OPEN, RF_BADPAIR = _lib.RF_EMPTY, _lib.RF_LPFAIL, _lib.RF_F1OPEN, _lib.RF_BADPAIR
_RF_NO_ROWS = RF_EMPTY | RF_LPFAIL | RF_F1OPEN   # plp_fm_emit writes no rows under these


def _pair_chunk(m_max, d, chunk):
    """Pairs per chunk: the caller's, or the library's default for this table shape (plp_pair_chunk_default: the one
    statement of that rule, csrc/plp_capi.hip)."""
    if chunk is not None and int(chunk) > 0:
        return int(chunk)
    return int(_lib.load().plp_pair_chunk_default(int(m_max), int(d)))


def _pair_table(what, A, b, m, pairs):
    """The table and the list of a listed-pair call -> (backend, A, b, m, n, m_max, d, pairs int32[K, 2], K)."""
    be, A, b, m, n, m_max, d = _cells(what, A, b, m)
    if m_max < 1 or 2 * m_max > MAX_M or d < 1 or d > MAX_D:
        raise _lib.UnsupportedSize("%s: m_max=%d d=%d outside envelope (2*m_max<=64, d<=16)" % (what, m_max, d))
    pairs = be.arr(pairs, np.int32)
    if len(pairs.shape) != 2 or pairs.shape[1] != 2:
        raise ValueError("pairs must be [K, 2]")
    return be, A, b, m, n, m_max, d, pairs, int(pairs.shape[0])


def _popcount64(words):
    """Bits set per 64-bit word (numpy uint64 / int64 or torch int64 -- the same bits) -> int64 of the same shape."""
    x = words.view(np.int64) if isinstance(words, np.ndarray) else words
    x = x - ((x >> 1) & 0x5555555555555555)
    x = (x & 0x3333333333333333) + ((x >> 2) & 0x3333333333333333)
    x = (x + (x >> 4)) & 0x0F0F0F0F0F0F0F0F
    return ((x * 0x0101010101010101) >> 56) & 0xFF


def pair_stacks(A, b, pairs, m=None):
    """The stacks of listed cell pairs: for pair t = (pairs[t, 0], pairs[t, 1]) = (i, j) of the n cells A[n, m_max, d],
    b[n, m_max] what Polytope(np.vstack([A_i, A_j]), np.hstack([b_i, b_j])) holds (polytope.py:272-275) -- cell i's rows,
    then cell j's, each scaled by the reciprocal of its norm, rows of norm <= 1e-10 dropped -- formed on the device.
    -> dict(A[K, 2 m_max, d], b[K, 2 m_max], m int32[K]), a packed table every batch call takes; rows from m[t] on are zero.
    pairs int32[K, 2]; 2 * m_max <= 64, d <= 16.  numpy: an index outside [0, n) or a pair (i, i) raises ValueError; CUDA
    tensors (nothing synchronises): such a pair gets m = 0 and nothing of the table is read for it."""
    be, A, b, m, n, m_max, d, pairs, K = _pair_table("pair_stacks", A, b, m, pairs)
    W = 2 * m_max
    As, bs, ms = be.out((K, W, d), zero=True), be.out((K, W), zero=True), be.out((K,), np.int32, zero=True)
    be.call("plp_pair_stacks", n, m_max, d, A, b, m, K, pairs, As, bs, ms, h2d=(A, b, m, pairs))
    return dict(A=As, b=bs, m=ms)


def _emit_pair_rows(be, A, b, m, n, m_max, d, pairs, keep, flags, abs_tol, chunk, mo_max):
    """The rows of the results of listed pairs from the keep words and flags their reduce gave: per chunk the stacks are
    formed again (a copy kernel) and go through plp_fm_emit(col = -1) -> A[K, mo_max, d], b[K, mo_max], m[K]."""
    K, W = int(pairs.shape[0]), 2 * m_max
    Ao, bo, mo = be.out((K, mo_max, d), zero=True), be.out((K, mo_max), zero=True), be.out((K,), np.int32, zero=True)
    if K == 0:
        return Ao, bo, mo
    c = min(K, _pair_chunk(m_max, d, chunk))
    sA, sb, sm = be.out((c, W, d)), be.out((c, W)), be.out((c,), np.int32)   # one table for all chunks (every slot is written)
    for lo in range(0, K, c):
        hi = min(K, lo + c)
        k = hi - lo
        As, bs, ms = sA[:k], sb[:k], sm[:k]
        be.call("plp_pair_stacks", n, m_max, d, A, b, m, k, pairs[lo:hi], As, bs, ms, h2d=(A, b, m))
        be.call("plp_fm_emit", k, W, d, As, bs, ms, keep[lo:hi], 1, flags[lo:hi], -1, 0, float(abs_tol), int(mo_max),
                Ao[lo:hi], bo[lo:hi], mo[lo:hi])
    return Ao, bo, mo


def _pair_mo_max(be, keep, flags):
    """The largest number of rows a result has (one read-back), at least 1."""
    if int(keep.shape[0]) == 0:
        return 1
    cnt = _popcount64(keep)
    if be.torch is not None:
        cnt = be.torch.where((flags & _RF_NO_ROWS) != 0, be.torch.zeros_like(cnt), cnt)
    else:
        cnt = np.where((flags & _RF_NO_ROWS) != 0, 0, cnt)
    return max(1, int(cnt.max()))


def intersect_pairs(A, b, pairs, m=None, abs_tol=1e-7, rows=True, chunk=None, mo_max=None):
    """The intersections of listed cell pairs of a table, formed on the device: for pair t = (i, j) of the n cells
    A[n, m_max, d], b[n, m_max] exactly what reduce_batch returns for the stack pair_stacks forms -- what
    cells[i].intersect(cells[j]) reduces (polytope.py:255-275) -- in list order:
    -> dict(keep uint64[K] (bit s = stack row s; where ms[t] == m_i + m_j the first m_i bits are cell i's rows), flags, r,
            xc[K, d], nlp, ms int32[K] (rows of the stack)[, A[K, mo_max, d], b[K, mo_max], m int32[K]]).
    rows=True: the results' rows as a packed table (fm_emit(col=-1) of the stacks under keep / flags: the (b + 0.1) - 0.1 round
    trip of a minimal representation, one constructor pass; m = 0 under RF_EMPTY / RF_LPFAIL / RF_F1OPEN).  mo_max: None --
    the largest popcount(keep) of the list, ONE read-back; the stacks are then formed a second time, chunk by chunk, for the
    emission (a copy kernel; the LPs run once).  An int -- no read-back, one pass, and m = -1 for a result of more rows.
    The list is worked off in chunks of `chunk` pairs (None: 32 MiB of stacks): the stacks of the whole list are
    never resident.  pairs int32[K, 2], 2 * m_max <= 64, d <= 16.  numpy in: numpy out, an index outside [0, n) or a pair
    (i, i) raises ValueError; CUDA tensors in: resident tensors on torch's current stream, and such a pair gets flags =
    RF_EMPTY | RF_BADPAIR, keep = r = nlp = ms = m = 0, xc = NaN."""
    be, A, b, m, n, m_max, d, pairs, K = _pair_table("intersect_pairs", A, b, m, pairs)
    c = 0 if chunk is None else int(chunk)
    res = dict(keep=be.out((K,), np.uint64, zero=True), flags=be.out((K,), np.int32, zero=True), r=be.out((K,), zero=True),
               xc=be.out((K, d), zero=True), nlp=be.out((K,), np.int32, zero=True), ms=be.out((K,), np.int32, zero=True))
    outs = (None, None, None)
    if rows and mo_max is not None:
        mo_max = int(mo_max)
        if mo_max < 0:
            raise ValueError("intersect_pairs: mo_max must not be negative")
        outs = (be.out((K, mo_max, d), zero=True), be.out((K, mo_max), zero=True), be.out((K,), np.int32, zero=True))
    ptrs = outs
    if rows and mo_max == 0 and K:
        # (no row slots: the empty A / b have no address, and a NULL A_out would turn the emission off -- the library gets
        # a word it never writes to, and m says which results have rows: -1)
        dummy = be.out((1,), zero=True)
        ptrs = (dummy, dummy, outs[2])
    be.call("plp_intersect_pairs", n, m_max, d, A, b, m, float(abs_tol), K, pairs, c, res["keep"], res["flags"], res["r"],
            res["xc"], res["nlp"], res["ms"], 0 if mo_max is None else mo_max, *ptrs, h2d=(A, b, m, pairs))
    if rows and mo_max is None:
        outs = _emit_pair_rows(be, A, b, m, n, m_max, d, pairs, res["keep"], res["flags"], abs_tol, chunk,
                               _pair_mo_max(be, res["keep"], res["flags"]))
    if rows:
        res["A"], res["b"], res["m"] = outs
    return res


# ------------------------------------------------------------------------------------- distances of listed pairs
_PAIR_DIST_MAX_D = 4            # the kernel (csrc/plp_pair_dist.hip) holds a simplex of d + 1 <= 5 points in registers
_PAIR_DIST_TOL = 1e-10          # the gap test of csrc/plp_pair_dist.hpp, relative to E = max(1, |x|_inf, |y|_inf)
_PAIR_DIST_ROUNDS = 64          # rounds of the host iteration before it gives up (status 4)
PAIR_BAD = 255


def _hull_nearest_origin(W, lam):
    """Wolfe's sub-algorithm in numpy: W[n, d] (the last point new, lam[n - 1] = 0) -> (kept indices, lam on them) with
    sum lam_k W_k the point of conv(W) nearest to the origin, or (None, None) for a corral that is affinely dependent."""
    keep = np.arange(W.shape[0])
    lam = np.asarray(lam, dtype=float).copy()
    for _ in range(W.shape[0] + 2):
        V = W[keep]
        if keep.size == 1:
            return keep, np.ones(1)
        Em = (V[1:] - V[0]).T
        a, _, rank, _ = np.linalg.lstsq(Em, -V[0], rcond=None)
        if rank < keep.size - 1 or not np.all(np.isfinite(a)):
            return None, None
        al = np.concatenate([[1.0 - a.sum()], a])
        if np.all(al > 0.0):
            return keep, al
        neg = al <= 0.0
        den = lam - al
        ratio = np.where(neg & (den > 0.0), lam / np.where(den > 0.0, den, 1.0), np.where(neg, 0.0, np.inf))
        kz = int(np.argmin(ratio))
        lam = lam + ratio[kz] * (al - lam)
        lam[kz] = 0.0
        stay = lam > 0.0
        if not stay.any():
            return None, None
        keep, lam = keep[stay], lam[stay]
    return None, None


def _pair_dist_resolve(be, A, b, m, pairs, out):
    """Raw status 1 settled on the host (distance_pairs: resolve=True), written into the arrays of `out`: the iteration of
    csrc/plp_pair_dist.hpp in numpy, its support points from lpsolve_batch (two calls per round for all open pairs), which
    starts from no centre -- flat cells are settled too.  -> codes 0, 2 (a cell is empty), 3 (unbounded), 4."""
    host = (lambda a: a.cpu().numpy()) if be.torch is not None else (lambda a: a)
    open_ = np.nonzero(host(out["status"]) == 1)[0]
    if not open_.size:
        return
    d, m_max = A.shape[2], A.shape[1]
    ph = host(pairs)[open_].astype(np.int64)
    cells, inv = np.unique(ph, return_inverse=True)
    inv = inv.reshape(ph.shape)
    sel = cells if be.torch is None else be.torch.as_tensor(cells, device=be.device)
    Ah, bh = host(A[sel]), host(b[sel])
    mh = np.full(cells.size, m_max, np.int32) if m is None else np.clip(host(m[sel]), 0, m_max).astype(np.int32)
    live = np.arange(m_max)[None, :] < mh[:, None]
    fin = (np.isfinite(Ah).all(axis=2) | ~live).all(axis=1) & (np.isfinite(bh) | ~live).all(axis=1)
    Ah, bh = np.where(live[:, :, None], Ah, 0.0), np.where(live, bh, 0.0)
    n = open_.size
    res = dict(dist=np.full(n, np.nan), lb=np.full(n, np.nan), x=np.full((n, d), np.nan), y=np.full((n, d), np.nan),
               status=np.full(n, 4, np.int32))
    ci, cj = inv[:, 0], inv[:, 1]
    run = fin[ci] & fin[cj]
    u = np.zeros((n, d))
    u[:, 0] = 1.0
    W, P, Q, lam = [None] * n, [None] * n, [None] * n, [None] * n
    cur = [None] * n   # (dist, E, x, y) of the current simplex
    for _ in range(_PAIR_DIST_ROUNDS):
        act = np.nonzero(run)[0]
        if not act.size:
            break
        si = lpsolve_batch(u[act], Ah[ci[act]], bh[ci[act]], mh[ci[act]])
        sj = lpsolve_batch(-u[act], Ah[cj[act]], bh[cj[act]], mh[cj[act]])
        for q, t in enumerate(act):
            a, c = int(si["status"][q]), int(sj["status"][q])
            if a or c:
                res["status"][t] = 2 if 2 in (a, c) else (3 if 3 in (a, c) else 4)
                run[t] = False
                continue
            p, r = si["x"][q], sj["x"][q]
            w = p - r
            lbv = float(u[t] @ w)
            if cur[t] is not None and cur[t][0] - max(lbv, 0.0) <= _PAIR_DIST_TOL * cur[t][1]:
                dd, _, xx, yy = cur[t]
                res["dist"][t], res["lb"][t], res["x"][t], res["y"][t], res["status"][t] = dd, min(max(lbv, 0.0), dd), xx, yy, 0
                run[t] = False
                continue
            if W[t] is None:
                W[t], P[t], Q[t], lam[t] = w[None], p[None], r[None], np.zeros(1)
            else:
                if np.any(np.all(W[t] == w[None], axis=1)) or W[t].shape[0] > d:
                    run[t] = False   # a stall: status 4
                    continue
                W[t], P[t], Q[t], lam[t] = np.vstack([W[t], w]), np.vstack([P[t], p]), np.vstack([Q[t], r]), np.append(lam[t], 0.0)
            keep, l = _hull_nearest_origin(W[t], lam[t])
            if keep is None:
                run[t] = False
                continue
            W[t], P[t], Q[t], lam[t] = W[t][keep], P[t][keep], Q[t][keep], l
            xx, yy = l @ P[t], l @ Q[t]
            v = xx - yy
            dd = float(np.linalg.norm(v))
            E = max(1.0, float(np.max(np.abs(xx))), float(np.max(np.abs(yy))))
            fell = cur[t] is None or dd < cur[t][0]
            cur[t] = (dd, E, xx, yy)
            if dd <= _PAIR_DIST_TOL * E:
                res["dist"][t], res["lb"][t], res["x"][t], res["y"][t], res["status"][t] = dd, 0.0, xx, yy, 0
                run[t] = False
            elif not fell or W[t].shape[0] > d:
                run[t] = False
            else:
                u[t] = v / dd
    for k, v in res.items():
        if out.get(k) is None:
            continue
        if be.torch is not None:
            out[k][be.torch.as_tensor(open_, device=be.device)] = be.torch.as_tensor(v).to(be.device)
        else:
            out[k][open_] = v


def distance_pairs(A, b, pairs, m=None, xc=None, points=True, resolve=True):
    """Closest points and Euclidean distances of listed cell pairs of a table:  min |x - y|_2  s.t.  A_i x <= b_i,  A_j y <= b_j
    for pair t = (pairs[t, 0], pairs[t, 1]) = (i, j) of the n cells A[n, m_max, d], b[n, m_max], m[n] -- a GJK iteration per
    pair on the device, its support points from the support LP of support_batch, two lanes per pair (include/plp.h:
    plp_pair_dist; csrc/plp_pair_dist.hpp).  pairs int32[K, 2]; a pair may appear more than once, in either order.
    xc[n, d]: a strictly interior point per cell; None: cheby_ball_batch runs first -- a cell it finds infeasible gives
    status 2 for its pairs, one without a usable centre (r <= 0, r = inf, the LP not optimal) a NaN centre, which the kernel
    hands back as status 1 (as support_batch).
    -> dict(dist[K], lb[K], x[K, d], y[K, d] (None with points=False), status int32[K]); numpy in, numpy out; CUDA tensors
    in, tensors out on torch's current stream.  x lies in cell i, y in cell j, dist = |x - y|, lb <= dist the lower bound
    -h_i(-u) - h_j(u), u = (x - y) / dist, of the last round (0 where the cells meet).
    status: 0 settled -- dist - max(lb, 0) <= 1e-10 E or dist <= 1e-10 E with E = max(1, |x|_inf, |y|_inf), x and y inside
    every row to 1e-10 E on unit-scaled slack, which holds dist within 5e-10 of the extent above and 2e-10 E below the true
    distance (plp_pair_dist.hpp has the derivation); 2 a cell is empty; 3 a cell is unbounded in a direction the iteration
    asked for (a cell without rows is); 4 no convergence or an input that is not finite; 1 (only with resolve=False) not
    settled by the kernel.  dist = lb = x = y = NaN wherever the status is not 0.
    resolve=True (the default) settles raw status 1 on the host: the same iteration in numpy with support points from
    lpsolve_batch (the certified path, which needs no centre, so flat cells are settled too).
    numpy: an index outside [0, n) or a pair (i, i) raises ValueError; CUDA tensors (nothing synchronises, so the list is
    not read by the host): such a pair gets status 255 (PAIR_BAD), NaN outputs, and nothing of the table is read for it.
    d <= 4 and m_max <= 64 only: other shapes raise UnsupportedSize.  There is NO fallback kernel for them."""
    be = _Backend(A)
    A, b, m, (n, m_max, d) = _packed(be, A, b, m)
    # (inf / nan in numpy inputs: ValueError from the library, which checks them while staging -- plp_ctx_set_check_finite)
    pairs = be.arr(pairs, np.int32)
    if len(pairs.shape) != 2 or pairs.shape[1] != 2:
        raise ValueError("pairs must be [K, 2]")
    K = int(pairs.shape[0])
    if d > _PAIR_DIST_MAX_D or m_max > MAX_M:
        raise _lib.UnsupportedSize("distance_pairs: m_max=%d d=%d outside the shared-row kernel (m <= 64, d <= 4)" % (m_max, d))
    if K > 2 ** 31 - 1:
        raise _lib.UnsupportedSize("distance_pairs: K exceeds 2^31 - 1")
    out = dict(dist=be.out((K,), zero=True), lb=be.out((K,), zero=True), x=be.out((K, d), zero=True) if points else None,
               y=be.out((K, d), zero=True) if points else None, status=be.out((K,), np.int32, zero=True))
    if K == 0:
        return out
    if be.torch is None:
        bad = (pairs < 0) | (pairs >= n)
        bad = bad[:, 0] | bad[:, 1] | (pairs[:, 0] == pairs[:, 1])
        if bad.any():
            t = int(np.nonzero(bad)[0][0])
            raise ValueError("distance_pairs: pair %d = (%d, %d): indices must be two different cells of [0, %d)"
                             % (t, pairs[t, 0], pairs[t, 1], n))
    elif n == 0:   # (no table: every listed pair is a bad one, and the library writes nothing)
        out["status"].fill_(PAIR_BAD)
        for k in ("dist", "lb", "x", "y"):
            if out[k] is not None:
                out[k].fill_(float("nan"))
        return out
    xp = be.torch if be.torch is not None else np
    infeasible = None
    if xc is not None:
        xc = _support_input(be, xc)
        if tuple(xc.shape) != (n, d):
            raise ValueError("xc must be [n, d] = [%d, %d], got %s" % (n, d, list(xc.shape)))
    else:
        ball = cheby_ball_batch(A, b, m)
        r = ball["r"]
        ok = (ball["status"] == 0) & (r > 0) & (r < float("inf"))
        nan = float("nan") if be.torch is None else be.torch.full((), float("nan"), dtype=be.torch.float64, device=be.device)
        xc = xp.where(ok[:, None], ball["xc"], nan)
        infeasible = ball["status"] == 2
    be.call("plp_pair_dist", n, m_max, d, A, b, m, xc, K, pairs, out["dist"], out["lb"], out["x"], out["y"], out["status"],
            h2d=(A, b, m, xc, pairs))
    if infeasible is not None and bool(infeasible.any()):
        # (a list on the device may hold indices outside [0, n): those pairs keep their 255)
        pc = pairs.clip(0, n - 1) if be.torch is None else pairs.clamp(0, n - 1)
        hit = (infeasible[pc[:, 0].long() if be.torch is not None else pc[:, 0]] |
               infeasible[pc[:, 1].long() if be.torch is not None else pc[:, 1]]) & (out["status"] != PAIR_BAD)
        out["status"][hit] = 2
        for k in ("dist", "lb", "x", "y"):
            if out[k] is not None:
                out[k][hit] = float("nan")
    if resolve:
        _pair_dist_resolve(be, A, b, m, pairs, out)
    return out


def intersect_cross_sparse(A, b, n1, m=None, abs_tol=1e-7, boxes=None, max_candidates=1 << 24, chunk=None):
    """The overlay of two lists of cells in one table (n1 cells, then n - n1): the full-dimensional intersections a ∩ c of a
    cell a < n1 of the first list with a cell c of the second, without any n1 x n2 object.
    -> dict(pairs int32[K', 2]: (a, c), c counted from 0 as overlap_cross_sparse, sorted by (a, c); A[K', mo_max, d],
            b[K', mo_max], m[K']: the K' cells as a packed table; r[K'], xc[K', d]: their Chebyshev balls; open: the positions
            in 0..K' whose flags carry RF_F1OPEN -- no verdict from the fused reduce, no rows (m = 0), for the caller to
            resolve (polytope.py: _reduce_many does, through the verified stand-alone ball); flags[K']; ncand).
    Broad phase as overlap_cross_sparse (box_pairs in the cross form, nothing inflated; `boxes`: outer boxes of the cells,
    see adjacent_pairs_sparse), then per chunk of whole cells of at most max_candidates candidates intersect_pairs: a pair is
    kept iff its stack is not RF_EMPTY -- the reduce's own Chebyshev LP is the narrow phase, no pair LP is solved twice.  The
    cull is exact: a ball of radius > abs_tol in both cells lies in both boxes.  Rows are emitted for the kept pairs only.
    chunk: as in intersect_pairs.
    numpy in: numpy out; CUDA tensors in: resident tensors on torch's current stream."""
    n1 = int(n1)
    what = "intersect_cross_sparse"
    be, A, b, m, n, m_max, d = _cells(what, A, b, m)
    if m_max < 1 or 2 * m_max > MAX_M or d < 1 or d > MAX_D:
        raise _lib.UnsupportedSize("%s: m_max=%d d=%d outside envelope (2*m_max<=64, d<=16)" % (what, m_max, d))
    if n1 < 0 or n1 > n:
        raise ValueError("%s: n1 must lie in 0..n" % what)
    max_candidates = int(max_candidates)
    if max_candidates < 1:
        raise ValueError("%s: max_candidates must be at least 1" % what)
    xp = be.torch if be.torch is not None else np
    found = []
    ncand = 0
    if n1 > 0 and n1 < n:
        if boxes is None:
            lb, ub = _outer_boxes(be, A, b, m, 0.0)
        else:
            lb, ub = boxes
            if tuple(lb.shape) != (n, d) or tuple(ub.shape) != (n, d):
                raise ValueError("%s: boxes must be (lb[n, d], ub[n, d])" % what)
        bp = _BoxPairs(be, lb, ub, n1, _LOCATE_PAD, "auto")
        ncand = bp.K
        for lo, hi in bp.chunks(max_candidates):
            cand = bp.fill(lo, hi)
            res = intersect_pairs(A, b, cand, m, abs_tol, rows=False, chunk=chunk)
            fl = res["flags"]
            live = ((fl & RF_EMPTY) == 0) | ((fl & RF_F1OPEN) != 0)
            found.append((cand[live], res["keep"][live], fl[live], res["r"][live], res["xc"][live]))
    if not found:
        found = [(be.out((0, 2), np.int32, zero=True), be.out((0,), np.uint64, zero=True), be.out((0,), np.int32, zero=True),
                  be.out((0,), zero=True), be.out((0, d), zero=True))]
    cat = (lambda v: v[0]) if len(found) == 1 else (be.torch.cat if be.torch is not None else np.concatenate)
    pairs, keep, flags, r, xc = (cat([f[k] for f in found]) for k in range(5))
    pairs, keep, flags = be.arr(pairs, np.int32), be.arr(keep, np.uint64), be.arr(flags, np.int32)
    Ao, bo, mo = _emit_pair_rows(be, A, b, m, n, m_max, d, pairs, keep, flags, abs_tol, chunk, _pair_mo_max(be, keep, flags))
    opened = xp.nonzero((flags & RF_F1OPEN) != 0)
    opened = opened[0] if isinstance(opened, tuple) else opened[:, 0]
    out_pairs = pairs.clone() if be.torch is not None else pairs.copy()
    if int(out_pairs.shape[0]):
        out_pairs[:, 1] -= n1
    return {"pairs": out_pairs, "A": Ao, "b": bo, "m": mo, "r": r, "xc": xc, "open": opened, "flags": flags, "ncand": ncand}


def selftest(group_size):
    """Cross-lane primitive self-test -> (out_d[128], out_u[128]) (see plp_points.hip)."""
    lib = _lib.load()
    od = np.empty(128)
    ou = np.empty(128, np.uint32)
    _lib.check(lib.plp_selftest(_lib.context().handle, int(group_size), _ptr(od), _ptr(ou)), "plp_selftest")
    return od, ou


def region_diff_search(A, b, m, mi, abs_tol=1e-7):
    """The search of region_diff (polytope.py:2201-2281) run by the library on the table A[m + 2M, d], b[m + 2M]
    (poly's m rows, the cells' new rows, their negations; rows already unit length) with mi[j] new rows per cell.

    -> (pieces, stats): pieces = list of (kind, rows) in the reference's order, kind 0 = Polytope(A[rows], b[rows]) as
    is, 1 = reduce() of it; stats = dict(lps, batches).  One launch + one synchronisation per visited node; the LPs
    are gathered on the device from the resident table by row index (include/plp.h: plp_region_diff_search)."""
    lib = _lib.load()
    A = _np(A)
    b = _np(b).ravel()
    mi = _np(mi, np.int32).ravel()
    nrows, d = A.shape
    if nrows != m + 2 * int(mi.sum()) or b.size != nrows:
        raise ValueError("region_diff_search: table must have m + 2 * sum(mi) rows")
    _finite_or_raise("region_diff_search", A, b)
    h = C.c_void_p()
    _count_h2d(A, b)
    _lib.check(lib.plp_region_diff_search(_lib.context().handle, d, int(m), int(mi.size), _ptr(mi), _ptr(A), _ptr(b),
                                          float(abs_tol), C.byref(h)), "plp_region_diff_search")
    try:
        nl, nr, nlp, nb = C.c_int64(), C.c_int64(), C.c_int64(), C.c_int64()
        _lib.check(lib.plp_rdiff_result_sizes(h, C.byref(nl), C.byref(nr), C.byref(nlp), C.byref(nb)), "plp_rdiff_result_sizes")
        kind = np.empty(max(nl.value, 1), np.int32)
        off = np.empty(nl.value + 1, np.int32)
        rows = np.empty(max(nr.value, 1), np.int32)
        _lib.check(lib.plp_rdiff_result_copy(h, _ptr(kind), _ptr(off), _ptr(rows)), "plp_rdiff_result_copy")
    finally:
        lib.plp_rdiff_result_free(h)
    pieces = [(int(kind[k]), rows[off[k]:off[k + 1]].copy()) for k in range(nl.value)]
    return pieces, dict(lps=int(nlp.value), batches=int(nb.value))


# ------------------------------------------------------------------ region_diff, many searches in one launch
RD_OK, RD_OVERFLOW, RD_COVERED, RD_LONG, RD_BUDGET, RD_INDEX, RD_UNSUPPORTED = range(7)   # include/plp.h: PLP_RD_*
RD_MAX_CELLS, RD_MAX_NEW = 64, 127   # the widths of mi[B, .] and src[B, .]: the kernel's caps on N and M
_RD_P_MAX, _RD_R_MAX = 32, 1024      # what the first launch has room for when the caller does not say


def _host(a):
    return a.cpu().numpy() if _is_torch(a) else np.asarray(a)


def _rdiff_launch(be, A, b, m, dims, CA, Cb, mc, cdims, cell_off, cell_idx, abs_tol, max_lps, p_max, r_max):
    (B, m_max, d), (Nc, mc_max) = dims, cdims

    def zeros(shape):   # (a problem that ends early leaves its slots unwritten)
        return be.torch.zeros(shape, dtype=be.torch.int32, device=be.device) if be.torch is not None else np.zeros(shape, np.int32)
    res = dict(kind=zeros((B, p_max)), off=zeros((B, p_max + 1)), rows=zeros((B, r_max)), count=zeros((B,)), nrows=zeros((B,)),
               nlp=zeros((B,)), status=zeros((B,)), mi=zeros((B, RD_MAX_CELLS)), src=zeros((B, RD_MAX_NEW)))
    be.call("plp_region_diff_batch", B, m_max, d, A, b, m, Nc, mc_max, CA, Cb, mc, cell_off, cell_idx, float(abs_tol),
            int(max_lps), int(p_max), int(r_max), RD_MAX_CELLS, RD_MAX_NEW, res["kind"], res["off"], res["rows"], res["count"],
            res["nrows"], res["nlp"], res["status"], res["mi"], res["src"], h2d=(A, b, m, CA, Cb, mc, cell_off, cell_idx))
    return res


def region_diff_search_batch(A, b, m, CA, Cb, mc, cell_off, cell_idx, abs_tol=1e-7, p_max=None, r_max=None, max_lps=1 << 16):
    """B region_diff searches in one launch (include/plp.h: plp_region_diff_batch), one per wavefront: problem p is the
    minuend A[p] (m[p] rows) minus the cells cell_idx[cell_off[p] : cell_off[p + 1]], in that order, of the packed cell table
    CA[Nc, mc_max, d], Cb[Nc, mc_max], mc[Nc].  Rows are unit length already, the cells sorted as region_diff sorts them.

    -> dict(kind int32[B, p_max], off[B, p_max + 1], rows[B, r_max], count[B], nrows[B], nlp[B], status[B] (RD_*),
            mi[B, 64], src[B, 127]): the pieces of problem p as lists of its LOCAL table rows, in the reference's order
    (`region_diff_leaves` reads them); src[p, k] = the cell-table row c * mc_max + r of its new row k.
    With p_max and r_max given the call is enqueued and returns (numpy: blocks, as every host-pointer call); an
    RD_OVERFLOW problem then holds what fitted, and count / nrows say what it needs.  With either None it launches with
    room for 32 pieces / 1024 rows, reads the status, and launches once more for the RD_OVERFLOW problems only, sized by
    their count / nrows."""
    be = _Backend(A)
    A, b, m, dims = _packed(be, A, b, m)
    CA, Cb, mc, (Nc, mc_max, dc) = _packed(be, CA, Cb, mc, "CA")
    if dc != dims[2]:
        raise ValueError("region_diff_search_batch: minuends and cells must have the same dimension")
    B = dims[0]
    cell_off, cell_idx = be.arr(cell_off, np.int32, (B + 1,)), be.arr(cell_idx, np.int32)
    fixed = p_max is not None and r_max is not None
    p1, r1 = int(_RD_P_MAX if p_max is None else p_max), int(_RD_R_MAX if r_max is None else r_max)
    if p1 < 1 or r1 < 1:
        raise ValueError("region_diff_search_batch: p_max and r_max must be at least 1")
    res = _rdiff_launch(be, A, b, m, dims, CA, Cb, mc, (Nc, mc_max), cell_off, cell_idx, abs_tol, max_lps, p1, r1)
    if fixed or B == 0:
        return res
    sel = np.nonzero(_host(res["status"]) == RD_OVERFLOW)[0]
    if sel.size == 0:
        return res
    p2, r2 = max(p1, int(_host(res["count"])[sel].max())), max(r1, int(_host(res["nrows"])[sel].max()))
    off_h = _host(cell_off).astype(np.int64)
    pos = np.concatenate([np.arange(off_h[s], off_h[s + 1]) for s in sel]).astype(np.int64)
    off2 = np.concatenate([[0], np.cumsum(off_h[sel + 1] - off_h[sel])]).astype(np.int32)
    if be.torch is not None:
        ix, posx = be.torch.as_tensor(sel, device=be.device), be.torch.as_tensor(pos, device=be.device)
        off2 = be.torch.as_tensor(off2, device=be.device)
    else:
        ix, posx = sel, pos
    sub_dims = (int(sel.size), dims[1], dims[2])
    sub = _rdiff_launch(be, be.arr(A[ix]), be.arr(b[ix]), None if m is None else be.arr(m[ix], np.int32), sub_dims, CA, Cb, mc,
                        (Nc, mc_max), off2, be.arr(cell_idx[posx], np.int32), abs_tol, max_lps, p2, r2)
    for key, width in (("kind", p2), ("off", p2 + 1), ("rows", r2)):
        big = sub[key].new_zeros((B, width)) if be.torch is not None else np.zeros((B, width), np.int32)
        big[:, :res[key].shape[1]] = res[key]
        res[key] = big
    for key in res:
        res[key][ix] = sub[key]
    return res


def region_diff_leaves(res, p):
    """The pieces of problem p of a region_diff_search_batch result that were written -> [(kind, rows int32 array)]."""
    n = min(int(res["count"][p]), res["kind"].shape[1])
    off, rows, kind = _host(res["off"][p]), _host(res["rows"][p]), _host(res["kind"][p])
    for k in range(n):   # RD_OVERFLOW: what fits is written -- the pieces in front of the first that did not (off = -1)
        if off[k + 1] < 0:
            n = k
            break
    return [(int(kind[k]), rows[off[k]:off[k + 1]].copy()) for k in range(n)]


def _rdiff_unit_rows(A3, b2, m):
    """The constructor's row scaling as region_diff applies it to its table (polytope.py:1755-1760), elementwise on packed
    rows; rows past m[p] become 0 -> (An, bn, ok[B]: every live row has a norm above 1e-10)."""
    live = np.arange(A3.shape[1])[None, :] < m[:, None]
    norms = np.sqrt(np.sum(A3 * A3, 2))
    ok = np.all(~live | (norms > 1e-10), axis=1)
    scale = np.zeros_like(norms)
    use = live & (norms > 1e-10)
    scale[use] = 1 / norms[use]
    return np.where(live[:, :, None], A3, 0.0) * scale[:, :, None], np.where(live, b2, 0.0) * scale, ok


def _rdiff_prepare(A, b, m, CA, Cb, mc, cell_off, cell_idx, intersect_tol, order):
    """Steps 1-4 of region_diff_batch on numpy arrays: unit rows, the radius of every (minuend, listed cell) stack in one
    cheby_ball_batch, the cells below intersect_tol dropped, each problem's cells ordered by np.argsort(-Rc) on its own
    array (or by order[p]).  -> dict(A, b, m, CA, Cb, mc, cell_off, cell_idx (the ordered lists), Rc (per listed pair, in
    the caller's order), ok[B])."""
    A, b = _np(A), _np(b)
    B, m_max, d = A.shape
    CA, Cb = _np(CA), _np(Cb)
    Nc, mc_max = CA.shape[:2]
    m = np.full(B, m_max, np.int32) if m is None else _np(m, np.int32)
    mc = np.full(Nc, mc_max, np.int32) if mc is None else _np(mc, np.int32)
    cell_off, cell_idx = _np(cell_off, np.int64), _np(cell_idx, np.int64)
    An, bn, ok = _rdiff_unit_rows(A, b.reshape(B, m_max), m)
    CAn, Cbn, okc = _rdiff_unit_rows(CA, Cb.reshape(Nc, mc_max), mc)
    L = int(cell_off[B])
    owner = np.repeat(np.arange(B), np.diff(cell_off))
    Rc = np.zeros(L)
    if L:
        # the stack [minuend; cell] of every listed pair, the cell's rows right behind the minuend's
        cidx = cell_idx[:L]
        ok &= np.bincount(owner, weights=~okc[cidx], minlength=B) == 0
        R = m_max + mc_max
        r = np.arange(R)[None, :]
        mp, mcl = m[owner][:, None], mc[cidx][:, None]
        from_p, from_c = r < mp, (r >= mp) & (r < mp + mcl)
        rp, rc_ = np.minimum(r, max(m_max - 1, 0)), np.clip(r - mp, 0, max(mc_max - 1, 0))
        A3, b3 = np.zeros((L, R, d)), np.zeros((L, R))
        if m_max:
            A3 = np.where(from_p[:, :, None], An[owner[:, None], rp], A3)
            b3 = np.where(from_p, bn[owner[:, None], rp], b3)
        if mc_max:
            A3 = np.where(from_c[:, :, None], CAn[cidx[:, None], rc_], A3)
            b3 = np.where(from_c, Cbn[cidx[:, None], rc_], b3)
        out = cheby_ball_batch(A3, b3, m=(mp + mcl).ravel().astype(np.int32))
        Rc = np.where((out["status"] == 0) & (out["r"] >= 0), out["r"], 0.0)
    new_off, new_idx = [0], []
    for p in range(B):
        lo, hi = int(cell_off[p]), int(cell_off[p + 1])
        Rp = Rc[lo:hi]
        N = int(np.sum(Rp >= intersect_tol))
        perm = np.argsort(-Rp) if order is None or order[p] is None else np.asarray(order[p], dtype=int)
        new_idx.append(cell_idx[lo:hi][perm[:N]])
        new_off.append(new_off[-1] + N)
    return dict(A=An, b=bn, m=m, CA=CAn, Cb=Cbn, mc=mc, cell_off=np.asarray(new_off, np.int32),
                cell_idx=np.concatenate(new_idx).astype(np.int32) if new_idx else np.zeros(0, np.int32), Rc=Rc, ok=ok)


def _rdiff_gather(pre, res):
    """The pieces of every problem as rows of the unit tables -> (status[B]: RD_UNSUPPORTED where a live row had no norm,
    else the search's; leaves: per problem the list of (kind, A[rows, d], b[rows]) of an RD_OK problem, else [])."""
    An, bn, mm = pre["A"], pre["b"], pre["m"]
    B, m_max, d = An.shape
    CAf, Cbf = pre["CA"].reshape(-1, d), pre["Cb"].ravel()
    status = np.where(pre["ok"], _host(res["status"]), RD_UNSUPPORTED).astype(np.int32)
    mi, src_all = _host(res["mi"]), _host(res["src"])
    leaves = []
    for p in range(B):
        mine = []
        if status[p] == RD_OK:
            m, M = int(mm[p]), int(mi[p].sum())
            # the problem's table: the minuend's rows, the new rows by `src`, their negations (the bits of numpy's -A)
            src = src_all[p, :M].astype(np.int64)
            TA = np.concatenate([An[p, :m], CAf[src], -CAf[src]])
            Tb = np.concatenate([bn[p, :m], Cbf[src], -Cbf[src]])
            mine = [(kind, TA[rows], Tb[rows]) for kind, rows in region_diff_leaves(res, p)]
        leaves.append(mine)
    return status, leaves


_RD_REDUCE_TOL = 1e-7   # region_diff reduces its leaves with the module's ABS_TOL whatever its own abs_tol (polytope.py)


def region_diff_batch(A, b, m, CA, Cb, mc, cell_off, cell_idx, abs_tol=1e-7, intersect_tol=1e-7, order=None):
    """Everything region_diff (polytope.py) does around its search, for B problems on packed numpy arrays: problem p is the
    minuend A[p] minus the union of the cells cell_idx[cell_off[p] : cell_off[p + 1]] of CA[Nc, mc_max, d], Cb, mc.
    Rows are scaled to unit length; the radius Rc of every (minuend, listed cell) stack comes from ONE cheby_ball_batch;
    cells with Rc < intersect_tol are dropped and the rest ordered by np.argsort(-Rc) on the problem's own array (`order`:
    a list with a permutation of a problem's list, or None, per problem, instead); the searches run in one launch
    (region_diff_search_batch); the pieces are gathered from the unit rows, and the pieces the reference reduce()s go
    through ONE reduce_batch and come back as reduce() leaves them: the kept rows, their right-hand sides through the
    reference's + 0.1 - 0.1 round trip where the reduce ran to the end, the rows scaled as the Polytope constructor scales
    them; a piece that reduces to the empty set is dropped, as region_diff's union drops it.

    -> dict(A[P, rows, d], b[P, rows], m[P]: the pieces of all problems; kind[P]: 0 = a piece as the search left it,
            1 = reduced, 2 = still to be reduce()d by the caller (the fused reduce's Chebyshev LP gave no verdict: rows as
            the search left them); piece_off[B + 1]: problem p owns pieces piece_off[p] : piece_off[p + 1]; status[B]
            (RD_*), Rc (per listed pair, in the caller's order), nlp[B]).
    A problem none of whose cells intersects returns its minuend (unit rows) as its one piece; one with a status other
    than RD_OK returns no piece (RD_COVERED: the difference is empty; the others are for the caller to solve another way:
    polytope.region_diff_batch sends them through region_diff)."""
    pre = _rdiff_prepare(_host(A), _host(b), None if m is None else _host(m), _host(CA), _host(Cb),
                         None if mc is None else _host(mc), _host(cell_off), _host(cell_idx), intersect_tol, order)
    d = pre["A"].shape[2]
    res = region_diff_search_batch(pre["A"], pre["b"], pre["m"], pre["CA"], pre["Cb"], pre["mc"], pre["cell_off"],
                                   pre["cell_idx"], abs_tol)
    status, leaves = _rdiff_gather(pre, res)
    flat = [(p, kind, Ak, bk) for p, mine in enumerate(leaves) for kind, Ak, bk in mine]
    red = [k for k, piece in enumerate(flat) if piece[1] == 1]
    dropped = set()
    kinds = [piece[1] for piece in flat]
    if red:   # the leaves the reference reduces (ref :2276), all problems' in one launch
        rm = np.array([flat[k][2].shape[0] for k in red], dtype=np.int32)
        RA, Rb = np.zeros((len(red), int(rm.max()), d)), np.zeros((len(red), int(rm.max())))
        for j, k in enumerate(red):
            RA[j, :rm[j]], Rb[j, :rm[j]] = flat[k][2], flat[k][3]
        out = reduce_batch(RA, Rb, m=rm, abs_tol=_RD_REDUCE_TOL)
        masks = keep_to_bool(out["keep"], RA.shape[1])
        for j, k in enumerate(red):
            fl = int(out["flags"][j])
            if fl & _lib.RF_LPFAIL:
                raise RuntimeError("bounding_box: an LP of the box prefilter of `reduce` ended with status 1 or 4")
            if fl & 32:   # PLP_RF_F1OPEN: reduce() re-examines these with verified LPs (polytope._reduce_many)
                kinds[k] = 2
                continue
            if fl & _lib.RF_EMPTY:
                dropped.add(k)
                continue
            keep = np.nonzero(masks[j, :rm[j]])[0]
            Ak, bk = flat[k][2][keep], flat[k][3][keep]
            if fl & _lib.RF_MINREP:
                bk = (bk + 0.1) - 0.1   # the h[k] += 0.1; h[k] -= 0.1 round trip of ref :1149-1151
            norms = np.sqrt(np.add.reduce(Ak * Ak, 1))   # the constructor's scaling (Polytope.__init__)
            if Ak.size and np.minimum.reduce(norms) > 1e-10:
                scale = 1 / norms
                Ak, bk = Ak * scale[:, None], bk * scale
            flat[k] = (flat[k][0], 1, Ak, bk)
    keep_k = [k for k in range(len(flat)) if k not in dropped]
    owner = np.array([flat[k][0] for k in keep_k], dtype=np.int64)
    piece_off = np.concatenate([[0], np.cumsum(np.bincount(owner, minlength=len(leaves)))]).astype(np.int64) \
        if len(leaves) else np.zeros(1, np.int64)
    P = len(keep_k)
    pm = np.array([flat[k][2].shape[0] for k in keep_k], dtype=np.int32)
    rmax = int(pm.max()) if P else 0
    Ao, bo = np.zeros((P, rmax, d)), np.zeros((P, rmax))
    for q, k in enumerate(keep_k):
        Ao[q, :pm[q]], bo[q, :pm[q]] = flat[k][2], flat[k][3]
    return dict(A=Ao, b=bo, m=pm, kind=np.array([kinds[k] for k in keep_k], dtype=np.int32), piece_off=piece_off,
                status=status, Rc=pre["Rc"], nlp=_host(res["nlp"]))


# ------------------------------------------------------------------ envelope: the facet tests of many regions in one launch
ENV_OK, ENV_OPEN, ENV_UNSUPPORTED = range(3)   # include/plp.h: PLP_ENV_*
ENV_MAX_DIM, ENV_MAX_ROWS = 8, 63              # the kernel's caps on d and on the rows of a listed member


def envelope_outer_batch(A, b, m, reg_off, mem_idx=None, abs_tol=1e-7):
    """The facet tests of envelope() for B regions in one launch (include/plp.h: plp_envelope_batch), one list entry per
    wavefront.  The members of all regions are the packed table A[C, mc_max, d], b[C, mc_max], m[C] (None: mc_max rows
    each) of unit rows; region p lists the members mem_idx[reg_off[p] : reg_off[p + 1]] (mem_idx None: the members of region
    p are reg_off[p] .. reg_off[p + 1] - 1 themselves).  Two regions may list the same member.

    -> dict(outer uint64[L] (int64 with tensors: the same bits), status int32[L] (ENV_*), nlp int32[L]) per list entry w:
    bit ii of outer[w] is set when no other entry of w's list reaches beyond row ii of member mem_idx[w] by more than
    abs_tol.  ENV_OPEN: a row counted as outer has a test behind it whose radius was NaN or within (abs_tol / 2,
    2 * abs_tol); ENV_UNSUPPORTED: a listed member has no row or more than 63, an index lies outside the table, or no pair
    reg_off[p] <= w < reg_off[p + 1] <= L holds the entry -- nothing was run for it and outer is 0.  d > 8 raises.
    numpy arrays or CUDA tensors in, the same kind out (numpy: blocks, as every host-pointer call)."""
    be = _Backend(A)
    A, b, m, (Cn, mc_max, d) = _packed(be, A, b, m)
    reg_off = be.arr(reg_off, np.int32)
    if len(reg_off.shape) != 1 or reg_off.shape[0] < 1:
        raise ValueError("envelope_outer_batch: reg_off must be [B + 1]")
    B = int(reg_off.shape[0]) - 1
    mem_idx = be.arr(mem_idx, np.int32)
    if mem_idx is not None:
        L = int(mem_idx.shape[0])
    else:   # (one scalar read back with tensors: the length of the identity list)
        L = int(reg_off[B]) if B else 0
        if L < 0 or L > Cn:
            raise ValueError("envelope_outer_batch: without mem_idx, reg_off must end within the member table")
    outer, status, nlp = be.out((L,), np.uint64, zero=True), be.out((L,), np.int32, zero=True), be.out((L,), np.int32, zero=True)
    be.call("plp_envelope_batch", Cn, mc_max, d, A, b, m, B, reg_off, L, mem_idx, float(abs_tol), outer, status, nlp,
            h2d=(A, b, m, reg_off, mem_idx))
    return dict(outer=outer, status=status, nlp=nlp)


_DGESV = None


def _lapack_dgesv_pointer():
    """Address of the dgesv numpy.linalg.solve's results agree with bit for bit (scipy's LAPACK; checked in the
    tests), or None when scipy is not importable -- the library then uses its own LU."""
    global _DGESV
    if _DGESV is None:
        try:
            from scipy.linalg import cython_lapack
            cap = cython_lapack.__pyx_capi__["dgesv"]
            C.pythonapi.PyCapsule_GetName.restype = C.c_char_p
            C.pythonapi.PyCapsule_GetName.argtypes = [C.py_object]
            C.pythonapi.PyCapsule_GetPointer.restype = C.c_void_p
            C.pythonapi.PyCapsule_GetPointer.argtypes = [C.py_object, C.c_char_p]
            _DGESV = C.pythonapi.PyCapsule_GetPointer(cap, C.pythonapi.PyCapsule_GetName(cap)) or 0
        except Exception:
            _DGESV = 0
    return _DGESV or None


def quickhull_run(X0, simplex, abs_tol=1e-7):
    """Quickhull's main loop in the library (include/plp.h: plp_quickhull_run): X0[N, d] translated points, simplex =
    indices of the start simplex -> (normals[n, d], offsets[n], verts int64[n, d], stats) of the hull's facets in the
    reference's order."""
    lib = _lib.load()
    X0 = _np(X0)
    N, d = X0.shape
    simplex = np.ascontiguousarray(simplex, dtype=np.int64).ravel()
    if simplex.size != d + 1:
        raise ValueError("quickhull_run: the start simplex has d + 1 points")
    _finite_or_raise("quickhull_run", X0)
    h = C.c_void_p()
    rc = lib.plp_quickhull_run(_lib.context().handle, N, d, _ptr(X0), _ptr(simplex), float(abs_tol),
                               C.c_void_p(_lapack_dgesv_pointer()), C.byref(h))
    if rc:
        msg = lib.plp_quickhull_last_error().decode("utf-8", "replace")
        if "Singular matrix" in msg:
            raise np.linalg.LinAlgError("Singular matrix")
        if "identical vertices" in msg:
            raise RuntimeError(msg)
        _lib.check(rc, "plp_quickhull_run")
    try:
        nf, it, made = C.c_int64(), C.c_int64(), C.c_int64()
        lib.plp_qh_result_sizes(h, C.byref(nf), C.byref(it), C.byref(made))
        normals = np.empty((nf.value, d))
        offsets = np.empty(nf.value)
        verts = np.empty((nf.value, d), np.int64)
        lib.plp_qh_result_copy(h, _ptr(normals), _ptr(offsets), _ptr(verts))
    finally:
        lib.plp_qh_result_free(h)
    return normals, offsets, verts, dict(iterations=int(it.value), facets_made=int(made.value))


# ------------------------------------------------------------------------------------- projection (Fourier-Motzkin)
def _fm_call(emit, A, b, col, m=None, keep=None, flags=None, first=False, abs_tol=1e-7, mo_max=0):
    be = _Backend(A)
    A, b, m, (B, m_max, d) = _packed(be, A, b, m)
    flags = be.arr(flags, np.int32, (B,))
    if keep is not None:
        keep = be.arr(keep.reshape(keep.shape[0], -1) if be.torch is not None else keep, np.uint64, (B, -1))
    kw = 0 if keep is None else int(keep.shape[1])
    head = (B, m_max, d, A, b, m, keep, kw, flags, int(col), int(bool(first)), float(abs_tol))
    if not emit:
        count = be.out((B,), np.int32)
        be.call("plp_fm_count", *head, count)
        return count
    Ao, bo = be.out((B, mo_max, d - 1 if col >= 0 else d)), be.out((B, mo_max))
    mo = be.out((B,), np.int32)
    be.call("plp_fm_emit", *head, int(mo_max), Ao, bo, mo)
    return Ao, bo, mo


def fm_count(A, b, col, m=None, keep=None, flags=None, first=False, abs_tol=1e-7):
    """Rows one Fourier-Motzkin step on column `col` forms per polytope, |N| + |P| |Q| (include/plp.h: plp_fm_count).
    `keep` / `flags`: the reduce_batch result that produced the rows (only kept rows are read, and each gets what reduce()
    does to it on the way out); `first`: one more constructor pass (the copy() of projection_fm's first step)."""
    return _fm_call(False, A, b, col, m, keep, flags, first, abs_tol)


def fm_emit(A, b, col, mo_max, m=None, keep=None, flags=None, first=False, abs_tol=1e-7):
    """The rows of that step -> (A_out[B, mo_max, d - 1], b_out[B, mo_max], m_out[B]) in the reference's order, each scaled
    as Polytope() does; m_out = -1 where the step forms more than mo_max rows (include/plp.h: plp_fm_emit).  col < 0: no
    elimination, the staged rows themselves (d columns)."""
    return _fm_call(True, A, b, col, m, keep, flags, first, abs_tol, mo_max)


# status codes of projection_batch
PROJ_OK, PROJ_EMPTY, PROJ_INPUT, PROJ_RAISES, PROJ_LPFAIL = 0, 1, 2, 3, 4
# projection_fm calls reduce() / is_fulldim() with the module's tolerance, whatever projection() was given (ref :1940-1950)
_REDUCE_TOL = 1e-7

# what the last projection_batch call did (scripts/bench_projection.py): launches and device-to-host bytes per step
fm_stats = {}


def _keep_width(rows):
    """Keep words per polytope for a tensor of `rows` row slots: the step kernels read ceil(rows / 64) of them whatever
    the row counts in use (include/plp.h: kw >= ceil(m_max / 64))."""
    return max(1, (int(rows) + 63) // 64)


def _reduce_split(torch, Ao, bo, mo_h, sel, stats):
    """Fused reduce of the polytopes `sel` (host indices into Ao) whose rows Ao[k, :mo_h[k]] hold: the ones of up to 64 rows
    on the register-resident kernels, the longer ones on the LDS kernel, each group packed to its own row count.
    -> keep words int64[len(sel), W] with W = _keep_width(Ao.shape[1]) (the words travel with Ao to the next step),
    flags int32[len(sel)] (device)"""
    n = len(sel)
    dev = Ao.device
    m_sel = mo_h[sel]
    W = _keep_width(Ao.shape[1])
    keep = torch.zeros((n, W), dtype=torch.int64, device=dev)
    flags = torch.empty((n,), dtype=torch.int32, device=dev)
    for grp in (np.nonzero(m_sel <= MAX_M)[0], np.nonzero(m_sel > MAX_M)[0]):
        if grp.size == 0:
            continue
        rows = int(m_sel[grp].max())
        gi = torch.as_tensor(np.asarray(sel)[grp], device=dev)
        Ag = Ao.index_select(0, gi)[:, :rows].contiguous()
        bg = bo.index_select(0, gi)[:, :rows].contiguous()
        mg = torch.as_tensor(m_sel[grp].astype(np.int32), device=dev)
        res = reduce_batch(Ag, bg, m=mg, abs_tol=_REDUCE_TOL)
        stats["launches"] += 1
        gt = torch.as_tensor(grp, device=dev)
        kw = res["keep"].reshape(len(grp), -1)
        keep[gt, :kw.shape[1]] = kw
        flags[gt] = res["flags"]
    return keep, flags


def _fm_batch(A, b, m, cols, abs_tol, reduced, on_host, stats=None):
    # abs_tol: the P / Q / N split (projection_fm's own argument); the reductions use the module's tolerance
    """Fourier-Motzkin steps of projection_fm (polytope/polytope.py:1911-1952) on packed device tensors.  `cols`: columns to
    eliminate, highest first.  reduced[k]: the rows of polytope k are already what projection_fm copies (a minimal
    representation, or the output of reduce()); otherwise the first reduce() runs here, fused.  on_host(k, poly, cols_left,
    first): the host continuation for polytope k, given the Polytope about to be eliminated on cols_left.
    -> list of B entries, (status, A_k, b_k, minrep) for polytopes that ended early, None for those handed to on_host
    or finished in the last step, followed by (idx, A, b, m, minrep) of the latter (packed, host arrays) or None."""
    import torch
    from .polytope import Polytope, _max_rows_reduce
    B, m_max, d = A.shape
    dev = A.device
    stats = [] if stats is None else stats   # (one dict per phase: launches, device-to-host bytes)
    out = [None] * B
    idx = np.arange(B)                   # polytope of each row of the current tensors
    m_h = m.cpu().numpy().astype(np.int64)
    keep = flags = None
    min_h = np.zeros(B, bool)            # minrep of the polytope the last reduce() returned (reduced inputs: False)
    cur_A, cur_b, cur_m = A, b, m
    first = True
    red = np.asarray(reduced, dtype=bool)
    if red.any() and not red.all():
        raise ValueError("_fm_batch: a batch is either all reduced or all unreduced")
    if not red.all():
        st = dict(step="reduce", launches=0, d2h=0, t=time.perf_counter())
        sel = np.nonzero(~red)[0]
        keep_r, flags_r = _reduce_split(torch, A, b, m_h, sel, st)
        keep, flags = keep_r, flags_r
        fl_h = flags.cpu().numpy()
        min_h = (fl_h & _lib.RF_MINREP) != 0
        st["d2h"] += 4 * B
        stats.append(st)
        dead = _fm_flags(fl_h)
        for k in np.nonzero(dead == 1)[0]:
            out[k] = (PROJ_RAISES, None, None, False)   # reduce() returned Polytope(): the reference fails on poly.A[:, i]
        for k in np.nonzero(dead == 3)[0]:
            out[k] = (PROJ_LPFAIL, None, None, False)
        for k in np.nonzero(dead == 2)[0]:
            on_host(int(k), Polytope(A[k, :m_h[k]].cpu().numpy(), b[k, :m_h[k]].cpu().numpy(), normalize=False), list(cols),
                    None)
            out[k] = None
        live = np.nonzero(dead == 0)[0]
        idx = live
        min_h = min_h[live]
        if live.size < B:
            li = torch.as_tensor(live, device=dev)
            cur_A, cur_b, cur_m = A.index_select(0, li), b.index_select(0, li), m.index_select(0, li)
            keep, flags = keep.index_select(0, li), flags.index_select(0, li)
    d_cur = d
    for s, col in enumerate(cols):
        if idx.size == 0:
            break
        st = dict(step="col %d" % col, launches=0, d2h=0, t=time.perf_counter())
        stats.append(st)
        count = fm_count(cur_A, cur_b, int(col), m=cur_m, keep=keep, flags=flags, first=first, abs_tol=abs_tol)
        st["launches"] += 1
        cnt = count.cpu().numpy().astype(np.int64)
        st["d2h"] += 4 * idx.size
        cap = _max_rows_reduce(d_cur - 1)
        big = cnt > cap
        mo_max = int(cnt[~big].max()) if (~big).any() else 0
        Ao, bo, mo = fm_emit(cur_A, cur_b, int(col), max(mo_max, 1), m=cur_m, keep=keep, flags=flags, first=first,
                             abs_tol=abs_tol)
        st["launches"] += 1
        mo_h = mo.cpu().numpy().astype(np.int64)
        st["d2h"] += 4 * idx.size
        for t in np.nonzero(big)[0]:   # beyond what the fused reduce takes: this step's rows on their own, then the host
            k = int(idx[t])
            kp = None if keep is None else keep[t:t + 1]
            fp = None if flags is None else flags[t:t + 1]
            Ak, bk, mk = fm_emit(cur_A[t:t + 1], cur_b[t:t + 1], int(col), int(cnt[t]), m=cur_m[t:t + 1], keep=kp,
                                 flags=fp, first=first, abs_tol=abs_tol)
            st["launches"] += 1
            n = int(mk[0])
            on_host(k, Polytope(Ak[0, :n].cpu().numpy(), bk[0, :n].cpu().numpy(), normalize=False), list(cols[s + 1:]),
                    "reduce")
        ok = ~big & (mo_h > 0)
        for t in np.nonzero(~big & (mo_h <= 0))[0]:
            out[int(idx[t])] = (PROJ_EMPTY, None, None, False)   # no rows: is_fulldim(Polytope of no rows) is False
        sel = np.nonzero(ok)[0]
        if sel.size == 0:
            idx = sel
            break
        keep, flags = _reduce_split(torch, Ao, bo, mo_h, sel, st)
        fl_h = flags.cpu().numpy()
        st["d2h"] += 4 * sel.size
        dead = _fm_flags(fl_h)
        for t in np.nonzero(dead == 1)[0]:
            out[int(idx[sel[t]])] = (PROJ_EMPTY, None, None, False)
        for t in np.nonzero(dead == 3)[0]:
            out[int(idx[sel[t]])] = (PROJ_LPFAIL, None, None, False)
        for t in np.nonzero(dead == 2)[0]:
            k = int(idx[sel[t]])
            n = int(mo_h[sel[t]])
            on_host(k, Polytope(Ao[sel[t], :n].cpu().numpy(), bo[sel[t], :n].cpu().numpy(), normalize=False),
                    list(cols[s + 1:]), "reduce")
        live = np.nonzero(dead == 0)[0]
        si = torch.as_tensor(sel[live], device=dev)
        li = torch.as_tensor(live, device=dev)
        cur_A, cur_b = Ao.index_select(0, si), bo.index_select(0, si)
        cur_m = mo.index_select(0, si)
        keep, flags = keep.index_select(0, li), flags.index_select(0, li)
        min_h = ((fl_h & _lib.RF_MINREP) != 0)[live]
        idx = idx[sel[live]]
        first = False
        d_cur -= 1
    if idx.size:
        # the last reduce's output polytope: its kept rows through the constructor (col < 0: no elimination)
        st = dict(step="compact", launches=0, d2h=0, t=time.perf_counter())
        stats.append(st)
        cnt = fm_count(cur_A, cur_b, -1, m=cur_m, keep=keep, flags=flags, first=first, abs_tol=abs_tol)
        mo_max = max(int(cnt.max().item()), 1)
        Ao, bo, mo = fm_emit(cur_A, cur_b, -1, mo_max, m=cur_m, keep=keep, flags=flags, first=first, abs_tol=abs_tol)
        st["launches"] += 2
        mo_h = mo.cpu().numpy()
        Ah, bh = Ao.cpu().numpy(), bo.cpu().numpy()
        st["d2h"] += 4 * idx.size + 4 + Ah.nbytes + bh.nbytes
        out.append((idx, Ah, bh, mo_h, min_h))   # the polytopes finished here, packed
    else:
        out.append(None)
    return out


def _fm_flags(fl):
    """reduce_batch flags -> 0 go on, 1 empty (Polytope()), 2 re-examine on the host, 3 reduce() raises (RF_LPFAIL)."""
    fl = np.asarray(fl)
    dead = np.zeros(fl.shape, np.int8)
    dead[(fl & _lib.RF_EMPTY) != 0] = 1
    dead[(fl & 32) != 0] = 2   # RF_F1OPEN: the verified path of polytope._reduce_many decides
    dead[(fl & _lib.RF_LPFAIL) != 0] = 3
    return dead


# ------------------------------------------------------------ projection by the iterative hull: many polytopes in one launch
(PH_OK, PH_UNBOUNDED, PH_FLAT, PH_OVERFLOW_POINTS, PH_OVERFLOW_FACETS, PH_BUDGET, PH_LPFAIL,
 PH_NOCENTRE) = range(8)   # include/plp.h: PLP_PH_*
PH_MAX_POINTS, PH_MAX_KEEP, PH_MAX_FACETS = 64, 3, 128   # the kernel's caps: points held, kept coordinates, f_max


def _ph_fmax(k):
    """The upper-bound theorem for 64 points in R^k, k <= 3."""
    return 2 if k == 1 else (PH_MAX_POINTS if k == 2 else 2 * PH_MAX_POINTS - 4)


def projection_hull_batch(A, b, dim, m=None, xc=None, f_max=None, points=False, max_lps=4096):
    """The projections of B packed polytopes onto the coordinates `dim` (1-based and increasing, at most 3) by the
    iterative hull in one launch (include/plp.h: plp_project_hull_batch has the rule in words): one polytope per
    wavefront, its rows read once, every facet LP and every hull rebuild inside the kernel.  A[B, m_max, d], b[B, m_max],
    m[B]; d <= 16, m_max <= 64 (beyond: UnsupportedSize).  xc[B, d]: a strictly interior point per polytope; None: the
    Chebyshev centres (cheby_ball_batch runs first; a polytope whose LP does not end optimal with r > 0 gets
    PH_NOCENTRE and the kernel runs nothing for it).  f_max None: the upper-bound theorem for 64 points.

    -> dict(A[B, f_max, k] unit rows, b[B, f_max], on uint64[B, f_max], m[B]: the rows of the projection (NaN / 0 beyond m;
            written for PH_OK only), V[B, 64, k], nv[B]: the points the hull was built from, X[B, 64, d] (points=True): a
            point of the polytope above each of them, vmask uint64[B]: bit i set when point i lies on at least k rows
            (advisory: a near-duplicate tilted row can set the bit of a point inside an edge), nlp[B], status[B] (PH_*)).
    numpy arrays or CUDA tensors in, the same kind out (tensors: on torch's current stream; uint64 as the same bits in
    int64)."""
    be = _Backend(A)
    A, b, m, (B, m_max, d) = _packed(be, A, b, m)
    keep = np.ascontiguousarray(np.asarray(dim, dtype=np.int64).ravel() - 1, dtype=np.int32)
    k = int(keep.size)
    if k < 1 or np.any(keep < 0) or np.any(keep >= d) or np.any(np.diff(keep) <= 0):
        raise ValueError("projection_hull_batch: dim must be increasing coordinates within 1 .. d")
    f_max = _ph_fmax(min(k, PH_MAX_KEEP)) if f_max is None else int(f_max)
    if f_max < 1 or int(max_lps) < 0:
        raise ValueError("projection_hull_batch: f_max must be at least 1 and max_lps at least 0")
    if xc is None and B:
        if be.torch is None and m is not None:
            # (the host-pointer ball checks its whole input for inf / nan; what lies beyond m[p] is nobody's to read)
            used = np.arange(m_max)[None, :] < m[:, None]
            ball = cheby_ball_batch(np.where(used[:, :, None], A, 0.0), np.where(used, b, 0.0), m)
        else:
            ball = cheby_ball_batch(A, b, m)
        if be.torch is not None:
            usable = (ball["status"] == 0) & (ball["r"] > 0)
            xc = be.torch.where(usable[:, None], ball["xc"], be.torch.full((), float("nan"), dtype=ball["xc"].dtype,
                                                                          device=be.device))
        else:
            with np.errstate(invalid="ignore"):
                usable = (ball["status"] == 0) & (ball["r"] > 0)
            xc = np.where(usable[:, None], ball["xc"], np.nan)
    xc = be.arr(xc, shape=(B, d)) if xc is not None else be.out((B, d), zero=True)
    Ao, bo = be.out((B, f_max, k), zero=True), be.out((B, f_max), zero=True)
    on, count = be.out((B, f_max), np.uint64, zero=True), be.out((B,), np.int32, zero=True)
    V, nv = be.out((B, PH_MAX_POINTS, k), zero=True), be.out((B,), np.int32, zero=True)
    X = be.out((B, PH_MAX_POINTS, d), zero=True) if points else None
    vmask, nlp, status = be.out((B,), np.uint64, zero=True), be.out((B,), np.int32, zero=True), be.out((B,), np.int32, zero=True)
    be.call("plp_project_hull_batch", B, m_max, d, k, A, b, m, _HostStruct((C.c_int32 * k)(*[int(v) for v in keep])), xc,
            f_max, int(max_lps), Ao, bo, on, count, V, nv, X, vmask, nlp, status, h2d=(A, b, m, xc))
    res = dict(A=Ao, b=bo, on=on, m=count, V=V, nv=nv, vmask=vmask, nlp=nlp, status=status)
    if points:
        res["X"] = X
    return res


def _projection_hull(torch, A2, b2, mt, go, live, new_dim, abs_tol, outs, routed):
    """The iterative-hull solver of projection_batch for the polytopes live[go]: the centre, the kernel, the rows through
    one reduce_batch (as the reference's qhull() reduces); whatever the kernel does not settle -- every PH_* but
    PH_UNBOUNDED, a shape beyond its caps, a reduce without a verdict -- goes through projection(..., solver="iterhull")
    into `outs`.  -> the settled polytopes as one block, or None."""
    from . import polytope as _poly
    gi = torch.as_tensor(go, device=A2.device)
    Ag, bg, mg = A2.index_select(0, gi), b2.index_select(0, gi), mt.index_select(0, gi)
    n, rows, d = Ag.shape
    k = len(new_dim)
    order = np.argsort(new_dim, kind="stable")
    back = np.argsort(order, kind="stable")   # column j of the answer is sorted column back[j]
    m_h = mg.cpu().numpy()
    st = np.full(n, PH_LPFAIL, np.int32)
    block = None   # (positions within go, A, b, m) of the polytopes settled here, as _fm_batch returns its last step
    if 1 <= k <= PH_MAX_KEEP and d <= MAX_D and rows <= MAX_M and np.all(np.diff(new_dim[order]) > 0):
        res = projection_hull_batch(Ag, bg, new_dim[order] + 1, m=mg)
        st = res["status"].cpu().numpy()
        cnt = res["m"].cpu().numpy()
        ok = np.nonzero(st == PH_OK)[0]
        if ok.size:
            cmax = int(cnt[ok].max())
            oi = torch.as_tensor(ok, device=A2.device)
            RA = torch.nan_to_num(res["A"].index_select(0, oi)[:, :cmax]).contiguous()
            Rb = torch.nan_to_num(res["b"].index_select(0, oi)[:, :cmax]).contiguous()
            red = reduce_batch(RA, Rb, m=torch.as_tensor(cnt[ok], device=A2.device), abs_tol=_REDUCE_TOL)
            masks = keep_to_bool(red["keep"].cpu().numpy(), cmax) & (np.arange(cmax)[None, :] < cnt[ok][:, None])
            flags = red["flags"].cpu().numpy()
            RA_h, Rb_h = RA.cpu().numpy(), Rb.cpu().numpy()
            # (32: PLP_RF_F1OPEN) a reduce without a verdict: the single call
            st[ok[(flags & (_lib.RF_LPFAIL | _lib.RF_EMPTY | 32)) != 0]] = PH_LPFAIL
            # the kept rows of every polytope to the front, in their order; the answers of all settled polytopes as one block
            front = np.argsort(~masks, axis=1, kind="stable")
            RA_h = np.take_along_axis(RA_h, front[:, :, None], 1)[:, :, back]
            Rb_h = np.take_along_axis(Rb_h, front, 1)
            trip = (flags & _lib.RF_MINREP) != 0   # the h[k] += 0.1; h[k] -= 0.1 round trip of ref :1149-1151
            Rb_h[trip] = (Rb_h[trip] + 0.1) - 0.1
            mk = masks.sum(1).astype(np.int32)
            pad = np.arange(cmax)[None, :] >= mk[:, None]
            RA_h[pad], Rb_h[pad] = 0.0, 0.0
            sel = st[ok] == PH_OK
            w = max(int(mk[sel].max()) if sel.any() else 0, 1)
            block = (ok[sel], RA_h[sel][:, :w], Rb_h[sel][:, :w], mk[sel])
    Ag_h = bg_h = None
    for t in np.nonzero(st != PH_OK)[0]:
        kk = int(live[go[t]])
        if st[t] == PH_UNBOUNDED:
            outs[kk] = (PROJ_LPFAIL, None, None, False)
            continue
        if Ag_h is None:
            Ag_h, bg_h = Ag.cpu().numpy(), bg.cpu().numpy()
        routed[0] += 1
        try:
            q = _poly.projection(_poly.Polytope(Ag_h[t, :m_h[t]].copy(), bg_h[t, :m_h[t]].copy(), normalize=False),
                                 new_dim + 1, solver="iterhull", abs_tol=abs_tol)
        except Exception:   # (the reference's iterhull raises plain Exception for an LP it cannot use)
            outs[kk] = (PROJ_LPFAIL, None, None, False)
            continue
        outs[kk] = (PROJ_OK, q.A, q.b, q.minrep) if q.A.size > 0 else (PROJ_EMPTY, None, None, False)
    return block


def _projection_exists(torch, At, bt, m_h, live, del_dim, abs_tol, dev, status, t_exists):
    """The part of projection() in front of its solvers, for the polytopes `live` of a packed batch: the zero rows of a
    polytope with fewer rows than dimensions and the existence LP.  Marks PROJ_EMPTY in `status` and -> A2, b2, mt (the
    rows of the live polytopes as the solvers take them) and `go`: the positions within `live` that go on.  Shared by
    both solvers of projection_batch."""
    B, m_max, d = At.shape
    # fewer rows than dimensions: zero rows up to d (ref :1748-1755)
    rows = max(m_max, d)
    li = torch.as_tensor(live, device=dev)
    A2 = torch.zeros((live.size, rows, d), dtype=torch.float64, device=dev)
    b2 = torch.zeros((live.size, rows), dtype=torch.float64, device=dev)
    A2[:, :m_max] = At.index_select(0, li)
    b2[:, :m_max] = bt.index_select(0, li)
    m2 = np.maximum(m_h[live], d)
    short = np.nonzero(m_h[live] < d)[0]
    if short.size:
        r = torch.arange(rows, device=dev)[None, :] >= torch.as_tensor(m_h[live][short], device=dev)[:, None]
        st_ = torch.as_tensor(short, device=dev)
        A2[st_] = torch.where(r[:, :, None], torch.zeros((), dtype=torch.float64, device=dev), A2[st_])
        b2[st_] = torch.where(r, torch.zeros((), dtype=torch.float64, device=dev), b2[st_])
    mt = torch.as_tensor(m2.astype(np.int32), device=dev)
    # does the projection exist: the Chebyshev-style LP with the reference's norm (squared, and zeroed on the ROWS
    # del_dim: ref :1757-1766)
    norm = (A2 * A2).sum(2)
    norm[:, torch.as_tensor(del_dim, device=dev)] = 0
    c = torch.zeros((live.size, d + 1), dtype=torch.float64, device=dev)
    c[:, d] = -1
    sol = lpsolve_batch(c, torch.cat([A2, norm[:, :, None]], 2).contiguous(), b2, m=mt)
    lp_st = sol["status"].cpu().numpy()
    r_h = sol["x"][:, d].cpu().numpy()
    fm_stats["steps"].append(dict(step="exists", launches=1, d2h=12 * live.size, t=t_exists))
    empty = (lp_st != 0) | ~(r_h >= abs_tol)
    status[live[empty]] = PROJ_EMPTY
    go = np.nonzero(~empty)[0]
    return A2, b2, mt, go


def projection_batch(A, b, dim, m=None, abs_tol=1e-7, minrep=False, solver="fm"):
    """projection(P_k, dim, solver=solver) (polytope/polytope.py:1698-1769, :1911-1952) of B packed polytopes whose rows are
    what Polytope(...).A / .b hold.  A[B, m_max, d], b[B, m_max], m[B] as numpy arrays or CUDA tensors; `dim`: the
    coordinates kept, 1-based, as the reference takes them; minrep: the inputs are minimal representations (no first
    reduce).

    -> dict(A[B, mo, len(dim)], b[B, mo], m[B], status[B], routed, reexamined).  status: 0 the rows of the projection;
    1 Polytope(); 2 the input returned unchanged (no rows, or len(dim) > d; A / b then hold nothing); 3 the reference
    raises IndexError here (its first reduce() returned Polytope()); 4 reduce() raises RuntimeError here (RF_LPFAIL).
    abs_tol is the existence LP's, as in projection(); the eliminations and reductions use the module's 1e-7, as
    projection_fm does when projection() calls it.  `routed`: polytopes whose step formed more rows than
    the fused reduce takes and went on through the host's reduce(); `reexamined`: polytopes the fused reduce handed to
    the verified Chebyshev LP (RF_F1OPEN), which went on on the host likewise.  Numpy in, numpy out; tensors in, tensors
    out (on A's device).

    solver: "fm" (the default: Fourier-Motzkin, everything above); "iterhull": the iterative hull in one launch
    (projection_hull_batch) behind the same existence LP, its rows through one reduce_batch as the reference's qhull()
    reduces them -- the same keys and status codes, 4 also where the projection is unbounded (the reference's iterhull
    has no answer there); `routed` then counts the polytopes the kernel did not settle (more than 64 points, a flat
    projection, an LP without a verdict, a shape beyond its caps), which went through projection(..., solver="iterhull");
    None: the reference's choice for the whole call -- fm for at most two deleted coordinates, otherwise the hull.  Any
    other name raises ValueError.
    """
    import torch
    from . import polytope as _poly
    if solver not in ("fm", "iterhull", None):
        raise ValueError('projection_batch: solver must be "fm", "iterhull" or None, not %r' % (solver,))
    numpy_in = not _is_torch(A)
    if numpy_in:
        dev = torch.device("cuda", torch.cuda.current_device())
        At = torch.as_tensor(_np(A), device=dev)
        bt = torch.as_tensor(_np(b), device=dev)
    else:
        dev = A.device
        At, bt = A.to(torch.float64).contiguous(), b.to(torch.float64).contiguous()
    if At.ndim != 3:
        raise ValueError("A must be [B, m_max, d]")
    B, m_max, d = At.shape
    bt = bt.reshape(B, m_max)
    m_h = np.full(B, m_max, np.int64) if m is None else (
        np.asarray(m.cpu().numpy() if _is_torch(m) else m, dtype=np.int64).reshape(B))
    dim = np.array(dim).flatten()
    new_dim = dim - 1
    del_dim = np.setdiff1d(range(d), new_dim)
    status = np.full(B, PROJ_INPUT, np.int32)
    fm_stats.clear()
    fm_stats["steps"] = []
    t_exists = time.perf_counter()
    outs = [None] * B
    routed, reexamined = [0], [0]
    live = np.nonzero(m_h > 0)[0] if d >= len(dim) else np.zeros(0, np.int64)
    block = None
    if live.size:
        A2, b2, mt, go = _projection_exists(torch, At, bt, m_h, live, del_dim, abs_tol, dev, status, t_exists)
        hull = solver == "iterhull" or (solver is None and len(del_dim) > 2)
        if hull and go.size:
            block = _projection_hull(torch, A2, b2, mt, go, live, new_dim, abs_tol, outs, routed)
        cols = [int(i) for i in -np.sort(-del_dim)]

        def on_host(k, poly, cols_left, first):
            kk = int(live[go[k]])
            if first == "reduce":
                routed[0] += 1
            else:
                reexamined[0] += 1
            try:
                q = _poly._fm_host_continue(poly, cols_left, _REDUCE_TOL, first)
            except IndexError:
                outs[kk] = (PROJ_RAISES, None, None, False)
                return
            except RuntimeError:
                outs[kk] = (PROJ_LPFAIL, None, None, False)
                return
            outs[kk] = (PROJ_OK, q.A, q.b, q.minrep) if q.A.size > 0 else (PROJ_EMPTY, None, None, False)
        if go.size and not hull:
            gi = torch.as_tensor(go, device=dev)
            res = _fm_batch(A2.index_select(0, gi), b2.index_select(0, gi), mt.index_select(0, gi), cols, _REDUCE_TOL,
                            np.full(go.size, bool(minrep)), on_host, fm_stats["steps"])
            block = res.pop()
            for t, r in enumerate(res):
                if r is not None:
                    outs[int(live[go[t]])] = r
        for k in range(B):
            if outs[k] is not None:
                status[k] = outs[k][0]
    t_pack = time.perf_counter()
    dn = len(dim) if d >= len(dim) else d
    mo = np.zeros(B, np.int32)
    for k in range(B):
        if outs[k] is not None and outs[k][0] == PROJ_OK:
            mo[k] = outs[k][1].shape[0]
    if block is not None:
        where = live[go[block[0]]]
        mo[where] = block[3]
        status[where] = PROJ_OK
    mo_max = max(int(mo.max()) if B else 0, 1)
    Ao = np.zeros((B, mo_max, dn))
    bo = np.zeros((B, mo_max))
    if block is not None:
        w = block[1].shape[1]
        Ao[where, :w] = block[1]
        bo[where, :w] = block[2]
    for k in range(B):
        if outs[k] is not None and mo[k]:
            Ao[k, :mo[k]] = outs[k][1]
            bo[k, :mo[k]] = outs[k][2]
    res = dict(A=Ao, b=bo, m=mo, status=status, routed=routed[0], reexamined=reexamined[0])
    # host wall time of each phase (each ends in a device-to-host copy, i.e. a synchronisation): step k runs from its own
    # start to the next one's; `pack` is the output's assembly on the host
    steps = fm_stats["steps"]
    ends = [st_["t"] for st_ in steps[1:]] + [t_pack]
    for st_, end in zip(steps, ends):
        st_["ms"] = (end - st_.pop("t")) * 1e3
    steps.append(dict(step="pack", launches=0, d2h=0, ms=(time.perf_counter() - t_pack) * 1e3))
    if not numpy_in:
        for key in ("A", "b", "m", "status"):
            res[key] = torch.as_tensor(res[key], device=dev)
    return res
