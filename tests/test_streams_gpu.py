"""GPU: WHEN a device-pointer call reads its inputs, and on WHOSE stream (tests/test_batch_contract_gpu.py settled what it may
read in space).  batch.py and include/plp.h promise for every `_dev` entry point: the call is enqueued on the stream the
caller hands in (torch's current stream), nothing synchronises, the result is ordered like any other work on that stream.

1. the gate.  The input tensors hold a valid DECOY batch; on a fresh stream s a delay is enqueued, then the copy of the
   real batch into those tensors, then the call, then a clone of every output; only s is synchronised.  A kernel, memset
   or verifier launch that went to another stream runs before the copy and answers for the decoy.  Every clone equals the
   synchronised real answer bit for bit (every case here is one test_batch_contract_gpu.py holds to the same bits from the
   same inputs: its position-dependent engines need more than 16 000 members).  The two answers differ -- in every member
   where an output is a float per member, in at least a quarter of the entries where the outputs are verdicts or indices
   (contains, the pair calls, subset; likewise the hit counts, owners and cell indices of the point kernels) -- so an answer
   for the decoy cannot pass.  Three controls make the call on a second stream and must get the decoy's bits while the
   gate is still closed: the detector works, and the delay is long enough.  The runtime maps the streams of a process
   onto a few hardware queues, and streams that share one run in order: the gate's stream is one that was seen to run
   side by side with the default stream, the control's second stream one that runs side by side with the first
   (runs_apart), so that what the test tells apart by timing can be told apart.
2. lpsolve / cheby_ball / bbox (the verifier's per-stream scratch, its two list counters) and assign_batch at F = 9 (its
   per-stream partials) on two streams at once, the buffers growing out of step.
3. twenty streams: the 16-stream tables are emptied on the way.
4. 80 fused reduces in flight over the ring of 64 retry words, and the simplex counter switched on from the second stream.
5. contains_batch across streams: the one thresholds buffer of the context, its hand-over and its grow path.  Overlap is
   a matter of timing here: the section can only catch a missing hand-over when the kernels really overlap; it is kept
   because it is the only execution of that code.
6. the synchronised real answers of section 1 against the outside references of test_batch_contract_gpu.py (the oracle for
   the LP family, contains and the pair kernels, the oracle's simplex for support, the host builds for the enumeration
   kernels), 20 members each: "equal to the synchronised call" is anchored in this file.  plp_fm_*, plp_volume_hits and the
   chained Python calls have no outside reference there; assign, hull_reassign and locate take the oracle's, subset_batch
   its answer by construction.

One process, no captured graphs.  Importing this module touches no device."""
import concurrent.futures
import os
import sys
import time

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from polytope_amd import batch, solvers  # noqa: E402
from polytope_amd.synth import quickhull_workload  # noqa: E402
import contract_cases as cc  # noqa: E402
import extreme_host as xh  # noqa: E402
import hull_host as hh  # noqa: E402
import locate_host as LH  # noqa: E402
import support_host as sh  # noqa: E402
import volume_exact_host as vh  # noqa: E402
from test_batch_contract_gpu import (TOL, assert_same, cells, pair_matrices, raw_bbox, raw_cheby, raw_contains,  # noqa: E402
                                     raw_extreme, raw_fm, raw_hull, raw_lp, raw_pairs, raw_reduce, raw_support,
                                     raw_volume, reduce_vs_oracle, switches, to_dev)
from test_reduce_plan import FIELDS, plan as reduce_plan  # noqa: E402,F401 (a fixture: the compiled plan)
from test_volume_exact_gpu import raw as raw_vol_exact  # noqa: E402

pytestmark = pytest.mark.gpu

make = sh._soak_lane().make   # scripts/soak_lane.py: the families `dup` and `unbounded`
B = 257                       # members of a gated batch
CELLS = 33                    # cells of the pair calls
NPTS = 4096                   # points of the point kernels
NREF = 20                     # members held to the outside reference
# the fused reduce with a second pass at (16, 3): the lane kernel redoes what it hands back inside its one launch and
# uses no retry word, so PLP_REDUCE_RETRY_ALL alone reaches neither; PLP_REDUCE_LANE=0 gives the lane-group engine, whose
# launch is followed by the general kernel's second pass (asserted on the plan)
SECOND_PASS = {"PLP_REDUCE_RETRY_ALL": 1, "PLP_REDUCE_LANE": 0}


# ------------------------------------------------------------------------------------------------ plumbing
def host(res):
    """Tensors to numpy WITHOUT a device-wide synchronisation (the copy waits for the default stream only; the caller has
    synchronised the stream that produced them)."""
    return {k: (v.cpu().numpy() if hasattr(v, "cpu") else np.asarray(v)) for k, v in res.items() if v is not None}


def pick(res, keys):
    return {k: res[k] for k in keys}


def _crop(a, b):
    """Two arrays cut to their common shape beyond the first axis (v_max, f_max and the rows of a projection follow the data)."""
    sl = (slice(None),) + tuple(slice(0, min(x, y)) for x, y in zip(a.shape[1:], b.shape[1:]))
    return a[sl], b[sl]


def members_differ(x, y):
    """bool[B]: some float output of member p differs in its bits."""
    out = None
    for k in x:
        a, b = np.asarray(x[k]), np.asarray(y[k])
        if a.dtype.kind != "f" or a.ndim < 1 or a.shape[0] != b.shape[0]:
            continue
        a, b = _crop(a, b)
        d = (np.ascontiguousarray(a).view(np.uint64) != np.ascontiguousarray(b).view(np.uint64)).reshape(a.shape[0], -1).any(1)
        out = d if out is None else (out | d)
    return out


def share_differs(x, y, key):
    a, b = _crop(np.asarray(x[key]), np.asarray(y[key]))
    return float(np.mean(a != b))


class G:
    """One gated case: fn(**args) -> dict of outputs; `real` and `decoy`, two valid batches of one shape (arrays as numpy;
    what is no array is the same in both); `differ`: "members" or the outputs held to the quarter rule; `ref(want, real, R)`:
    the outside reference of section 6 (R: the oracle and the host builds); `prepare(case)`: what has to be read from the
    device before the shapes are known."""

    def __init__(self, fn, real, decoy, env=None, differ="members", ref=None, prepare=None):
        self.fn, self.real, self.decoy, self.env = fn, real, decoy, env or {}
        self.differ, self.ref, self.prepare = differ, ref, prepare
        assert set(real) == set(decoy)
        for k, v in real.items():
            if isinstance(v, np.ndarray):
                assert v.shape == decoy[k].shape and v.dtype == decoy[k].dtype, k
            else:
                assert v is decoy[k] or v == decoy[k], k

    def tensors(self, args):
        return {k: to_dev(v) for k, v in args.items()}


def bounded(m_max, d, seed, n=B, scale=1.0):
    """cc.mixed_rows without its special members: every member bounded with the origin inside, every float output its own.
    scale: the polytopes blown up about the origin (the shadow of a member on two axes is often the box |x_i| <= 3 alone:
    a decoy of another size differs from it there too)."""
    A, b, m = cc.mixed_rows(n, m_max, d, seed, bounded_only=True)
    return dict(A=A, b=b * scale, m=m)


def dup(seed, n=B, other=None):
    """The `dup` family at (16, 3); other: a batch whose box (one side for the whole batch) this one must not share."""
    while True:
        A, b, m = make(np.random.default_rng(seed), n, 16, 3, "dup")
        if other is None or np.median(b[:, :6]) != np.median(other["b"][:, :6]):
            return dict(A=A, b=b, m=m)
        seed += 1000


def unbounded(seed, n):
    """The `unbounded` family at (5, 3): five random half-spaces in R^3 are unbounded two times out of three (at 16 rows
    hardly ever), so the engines report LPs unbounded and the verifier hands them to the careful engine."""
    A, b, m = make(np.random.default_rng(seed), n, 5, 3, "unbounded")
    return dict(A=A, b=b, m=m)


# ------------------------------------------------------------------------------------------------ the gated cases
def lp_case(m_max, n, seed, shift):
    """shift: the polytope moved 6 away from the origin, so that some h_i < 0 in every member (lp_r_kernel hands it to
    lp_p1_r_kernel and lp_kernel: three launches and the verifier)."""
    G_, h, m = cc.mixed_rows(B, m_max, n, seed, bounded_only=True)
    rng = np.random.default_rng(seed + 1)
    c = rng.standard_normal((B, n))
    if shift:
        t = rng.standard_normal((B, n))
        t *= 6.0 / np.linalg.norm(t, axis=1, keepdims=True)
        h = h - np.einsum("pij,pj->pi", G_, t)
        live = np.arange(m_max)[None, :] < m[:, None]
        assert ((h < 0) & live).any(1).all()
    return dict(c=c, G=G_, h=h, m=m)


def ref_lp(want, a, R):
    assert (want["status"][:NREF] == 0).all()
    for k in range(NREF):
        mk = a["m"][k]
        so, _, fo, _ = R.O.lp_solve(a["c"][k], a["G"][k, :mk], a["h"][k, :mk])
        assert want["status"][k] == so, (k, want["status"][k], so)
        assert abs(want["fun"][k] - fo) <= TOL * max(1.0, abs(fo)), k
        assert np.max(a["G"][k, :mk] @ want["x"][k] - a["h"][k, :mk]) <= 1e-7


def ref_cheby(want, a, R):
    for k in range(NREF):
        mk = a["m"][k]
        so, ro, _ = R.O.cheby(a["A"][k, :mk], a["b"][k, :mk])
        assert want["status"][k] == so, (k, want["status"][k], so)
        if so == 0:
            assert abs(want["r"][k] - ro) <= TOL, (k, want["r"][k], ro)
            nrm = np.linalg.norm(a["A"][k, :mk], axis=1)
            assert np.max(a["A"][k, :mk] @ want["xc"][k] + nrm * want["r"][k] - a["b"][k, :mk]) <= 1e-9


def ref_bbox(want, a, R):
    for k in range(NREF):
        mk = a["m"][k]
        lb, ub, bad = R.O.bounding_box(a["A"][k, :mk], a["b"][k, :mk])
        r, _ = R.O.cheby_ball(a["A"][k, :mk], a["b"][k, :mk])
        if want["status"][k] == 0:
            assert bad == 0 and r >= 1e-6 - 1e-12, (k, r)
            assert np.allclose(want["lb"][k], lb.ravel(), rtol=0, atol=TOL), (k, want["lb"][k], lb.ravel())
            assert np.allclose(want["ub"][k], ub.ravel(), rtol=0, atol=TOL), (k, want["ub"][k], ub.ravel())
        else:
            assert want["status"][k] == 1 and r < 1e-6 + 1e-12, (k, r)
    assert (want["status"][:NREF] == 0).sum() > NREF // 2


def ref_reduce(want, a, R):
    reduce_vs_oracle(R.O, a, want, NREF)


def contains_case(P, seed, mode):
    X = np.random.default_rng(seed + 7).uniform(-2.3, 2.3, (3, NPTS))   # (about half the points inside a polytope)
    return dict(bounded(16, 3, seed, n=P), X=X, mode=mode)


def ref_contains(want, a, R):
    n = min(NREF, len(a["m"]))
    ref = np.stack([R.O.contains(a["A"][p:p + 1, :a["m"][p]], a["b"][p:p + 1, :a["m"][p]], np.ascontiguousarray(a["X"].T))[0]
                    for p in range(n)])
    if a["mode"] == 1:
        assert np.array_equal(want["out"][:n], ref) and 0 < ref.sum() < ref.size
    else:
        assert n == len(a["m"]) and np.array_equal(want["out"], ref.any(axis=0).astype(np.uint8))


def ref_pairs(want, a, R, tol=1e-7):
    """The rule of test_batch_contract_gpu.test_pairs_padding_members_oracle on every pair of the first 20 cells."""
    n, n1 = len(a["m"]), a["n1"]
    W = pair_matrices(want, n, n1)
    near = 0
    for i in range(NREF):
        for j in range(i):
            SA = np.vstack([a["A"][i, :a["m"][i]], a["A"][j, :a["m"][j]]])
            Sb = np.hstack([a["b"][i, :a["m"][i]], a["b"][j, :a["m"][j]]])
            for key, inflate, thresh in (("adj", tol, tol / 10), ("ov", 0.0, tol)):
                st, r, _ = R.O.cheby(SA, Sb + inflate)
                assert st != 0 or abs(r - thresh) > 1e-9, (i, j, key, r)
                yes = int(st == 0 and r > thresh)
                assert W[key][i, j] == yes, (i, j, key, st, r)
                near += yes
                assert W["rng" if key == "adj" else "cross"][i, j] in (-1, yes), (i, j, key)
    assert 0 < near < NREF * (NREF - 1)


def fm_prepare(case):
    """mo_max: the largest count of either batch (plp_fm_count on both, synchronised)."""
    import torch
    most = 1
    for args in (case.real, case.decoy):
        count = raw_fm(**case.tensors(dict(args, mo_max=1)))["count"]
        torch.cuda.synchronize()
        most = max(most, int(count.max()))
    case.real["mo_max"] = case.decoy["mo_max"] = most


def volume_case(seed):
    a = bounded(11, 3, seed)
    state, inc = batch._pcg64_words([1000 * seed + p for p in range(B)])
    return dict(a, lb=np.full((B, 3), -3.1), ub=np.full((B, 3), 3.1), state=state, inc=inc, N=777)


def support_case(seed):
    return dict(bounded(16, 3, seed), Cd=np.random.default_rng(seed).standard_normal((5, 3)), shared=1, xc=np.zeros((B, 3)))


def ref_support(want, a, R):
    A, b, m = a["A"][:NREF], a["b"][:NREF], a["m"][:NREF]
    ost, oh, ox = sh.oracle_support(R.O, A, b, m, a["Cd"], extent=True)
    st = want["status"][:NREF]
    assert set(np.unique(st)) <= {0, 1, 3} and (st == 0).mean() > 0.8
    sh.check_against_oracle(A, b, m, a["Cd"], want["h"][:NREF], want["x"][:NREF], st, ost, oh, where=(st != 1), ext=ox)


def ref_extreme(want, a, R):
    V, count, bas, status = xh.run(R.xh, a["A"][:NREF], a["b"][:NREF], a["m"][:NREF], None, a["v_max"])
    assert np.array_equal(want["status"][:NREF], status) and np.array_equal(want["count"][:NREF], count)
    assert (status == xh.XS_OK).all() and np.array_equal(want["basis"][:NREF], bas) and cc.same_bits(want["V"][:NREF], V)


def points_case(seed):
    """cc.mixed_points without its five special members and without the sets of fewer than six points (four points with an
    exact repeat among them are flat): the first B of the rest, every one with a hull."""
    X, n = cc.mixed_points(2 * B + 5, 16, 3, seed)
    sel = (5 + np.nonzero(n[5:] >= 6)[0])[:B]
    assert len(sel) == B
    return dict(X=np.ascontiguousarray(X[sel]), n=np.ascontiguousarray(n[sel]))


def ref_hull(want, a, R):
    ref = hh.run(R.hh, a["X"][:NREF], a["n"][:NREF], None, a["f_max"])
    assert (ref["status"] == hh.HS_OK).all()
    got = {k: (v[:NREF].view(np.uint64) if k == "on" else v[:NREF]) for k, v in want.items()}
    assert hh.same_result(got, ref) is None, hh.same_result(got, ref)


def ref_vol_exact(want, a, R):
    vol, area, status = vh.run(R.vh, a["A"][:NREF], a["b"][:NREF], a["m"][:NREF])
    assert (status == vh.VS_OK).all() and np.array_equal(want["status"][:NREF], status)
    assert cc.same_bits(want["volume"][:NREF], vol) and cc.same_bits(want["area"][:NREF], area)


def assign_case(F, seed):
    X, nrm, off = quickhull_workload(NPTS, d=3, F=F, seed=seed)
    return dict(X=X, normals=nrm, offsets=off)


def ref_assign(want, a, R):
    fo, do_, am, mx = R.O.assign(a["X"], a["normals"], a["offsets"], 1e-7)
    assert np.array_equal(want["facet"], fo) and np.array_equal(want["dist"], do_) and np.array_equal(want["argmax"], am)
    assert np.array_equal(want["maxd"][am >= 0], mx[am >= 0]) and (am >= 0).any() and (fo < 0).any()


def reassign_case(seed):
    """The first update of a hull session: every point is owned by facet 0, which dies; five new facets."""
    rng = np.random.default_rng(seed)
    nrm = rng.standard_normal((5, 3))
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    dead = np.zeros(64, np.uint8)
    dead[0] = 1
    return dict(X=rng.standard_normal((NPTS, 3)), owner=np.zeros(NPTS, np.int32), dist=np.zeros(NPTS), dead=dead,
                normals=nrm, offsets=0.8 * rng.random(5))


def run_reassign(X, owner, dist, dead, normals, offsets):
    owner, dist = owner.clone(), dist.clone()   # (updated in place: the case's tensors stay what they were)
    return dict(batch.hull_reassign_dev(X, owner, dist, dead, 1, normals, offsets, 1e-7), owner=owner, dist=dist)


def ref_reassign(want, a, R):
    owner, dist = a["owner"].copy(), a["dist"].copy()
    cnt, am, mx = R.O.hull_reassign(a["X"], owner, dist, a["dead"], 1, a["normals"], a["offsets"], 1e-7)
    assert np.array_equal(want["owner"], owner) and np.array_equal(want["dist"], dist)
    assert np.array_equal(want["count"], cnt) and np.array_equal(want["argmax"], am) and cnt.sum() > 0
    assert np.array_equal(want["maxd"][am >= 0], mx[am >= 0])


def locate_case(seed):
    rng = np.random.default_rng(seed)
    A, b = LH._cells_table(3, 5, rng, jitter=0.4)   # 125 overlapping cells: lists of several entries
    return dict(A=A, b=b, X=LH._points(rng, 3, NPTS, 1.2))


def run_locate(A, b, X):
    """locate_grid (plp_bbox_batch, plp_locate_grid_count, a read-back, plp_locate_grid_fill) and plp_locate on its lists."""
    g = batch.locate_grid(A, b)
    assert g.kind == "grid" and g.max_list > 1, g
    first, count = batch.locate_batch(A, b, X, count=True, grid=g)
    return dict(first=first, count=count, cell_start=g.cell_start, cell_items=g.cell_items)


def ref_locate(want, a, R):
    """The definition in locate_batch's docstring on 200 points: the first polytope the oracle's contains has the point in."""
    inside = R.O.contains(a["A"], a["b"], np.ascontiguousarray(a["X"][:, :200].T))
    first = np.where(inside.any(0), inside.argmax(0), -1)
    assert np.array_equal(want["first"][:200], first) and np.array_equal(want["count"][:200], inside.sum(0))
    assert (first >= 0).any() and (first < 0).any()


def with_hip(fn):
    def run(**kw):
        saved, solvers.default_solver = solvers.default_solver, "hip"
        try:
            return fn(**kw)
        finally:
            solvers.default_solver = saved
    return run


def subset_case(seed, shrink):
    """Q = P blown up (P <= Q), but moved inwards for every second member, starting at `shrink` (P is not in Q)."""
    A, b, m = cc.mixed_rows(B, 12, 3, seed, bounded_only=True)
    Qb = b * 1.5
    Qb[shrink::2] = b[shrink::2] - 1.5
    return dict(A=A, b=b, m=m, QA=A.copy(), Qb=Qb, mq=np.random.default_rng(seed).integers(1, 13, B).astype(np.int32))


def ref_subset(want, a, R):
    """By construction: P lies in 1.5 P; the ball of radius 1 about the origin lies in P and not behind a row of Q = the
    rows of P moved 1.5 inwards that was tangent to a sphere of radius <= 2 (the rows from 7 on)."""
    sub, p = want["sub"].astype(bool), np.arange(B)
    assert sub[p % 2 == 1].all() and not sub[(p % 2 == 0) & (a["mq"] >= 7)].any()


SUPPORT_C = np.random.default_rng(5).standard_normal((5, 3))
VOLUME_SEEDS = list(range(B))


def build_cases():
    d1 = dup(11)
    hull_a, hull_b = points_case(43), points_case(44)
    fmax = hh.fmax_for(3, 16)
    v16 = xh.vmax_for(3, 16)
    return {
        "lp-n3-phase1": G(raw_lp, lp_case(16, 3, 1, True), lp_case(16, 3, 2, True), ref=ref_lp),
        "lp-n8": G(raw_lp, lp_case(24, 8, 3, False), lp_case(24, 8, 4, False), ref=ref_lp),
        "cheby-dup": G(raw_cheby, d1, dup(12, other=d1), ref=ref_cheby),
        "bbox-dup": G(raw_bbox, d1, dup(12, other=d1), ref=ref_bbox),
        "reduce-second-pass": G(raw_reduce, bounded(16, 3, 5), bounded(16, 3, 6), env=SECOND_PASS, ref=ref_reduce),
        "reduce-wide-70": G(raw_reduce, bounded(70, 3, 7), bounded(70, 3, 8), ref=ref_reduce),
        "contains-per-polytope": G(raw_contains, contains_case(B, 9, 1), contains_case(B, 10, 1), differ=("out",), ref=ref_contains),
        "contains-region": G(raw_contains, contains_case(2, 9, 0), contains_case(2, 10, 0), differ=("out",), ref=ref_contains),
        "pairs": G(raw_pairs, dict(cells(CELLS, 10, 4, seed=13), n1=12), dict(cells(CELLS, 10, 4, seed=14), n1=12),
                   differ=("adj", "rng", "ov", "cross"), ref=ref_pairs),
        "fm": G(raw_fm, dict(bounded(10, 3, 15), keep=None, flags=None, col=2, first=0, mo_max=1),
                dict(bounded(10, 3, 16), keep=None, flags=None, col=2, first=0, mo_max=1), prepare=fm_prepare),
        "volume-hits": G(raw_volume, volume_case(17), volume_case(18), differ=("hits",)),
        "support": G(raw_support, support_case(19), support_case(20), ref=ref_support),
        "extreme": G(raw_extreme, dict(bounded(16, 3, 21), keep=None, v_max=v16), dict(bounded(16, 3, 22), keep=None, v_max=v16),
                     ref=ref_extreme),
        "hull": G(raw_hull, dict(hull_a, keep=None, f_max=fmax), dict(hull_b, keep=None, f_max=fmax), ref=ref_hull),
        "vol-exact": G(raw_vol_exact, bounded(16, 3, 23), bounded(16, 3, 24), ref=ref_vol_exact),
        "assign-F9": G(lambda **kw: batch.assign_batch(abs_tol=1e-7, **kw), assign_case(9, 25), assign_case(9, 26),
                       differ=("facet", "dist"), ref=ref_assign),
        "assign-F600": G(lambda **kw: batch.assign_batch(abs_tol=1e-7, **kw), assign_case(600, 27), assign_case(600, 28),
                         differ=("facet", "dist"), ref=ref_assign),
        "hull-reassign": G(run_reassign, reassign_case(29), reassign_case(30), differ=("owner", "dist"), ref=ref_reassign),
        "locate-grid": G(run_locate, locate_case(31), locate_case(32), differ=("first",), ref=ref_locate),
        # the Python calls that chain launches and read-backs
        "py-projection": G(with_hip(lambda A, b, m: pick(batch.projection_batch(A, b, [1, 2], m=m), ("A", "b", "m", "status"))),
                           bounded(12, 4, 33), bounded(12, 4, 34, scale=1.25)),
        "py-extreme-reduce": G(lambda A, b, m: pick(batch.extreme_batch(A, b, m=m), ("V", "count", "status")),
                               bounded(16, 3, 35), bounded(16, 3, 36)),
        "py-volume-exact-reduce": G(lambda A, b, m: pick(batch.volume_exact_batch(A, b, m=m), ("volume", "area", "status")),
                                    bounded(16, 3, 37), bounded(16, 3, 38)),
        "py-volume-own-boxes": G(lambda A, b, m: pick(batch.volume_batch(A, b, m=m, nsamples=500, seed=VOLUME_SEEDS),
                                                      ("volume", "hits", "lb", "ub", "flags")),
                                 bounded(12, 3, 39), bounded(12, 3, 40)),
        "py-support-resolve": G(lambda A, b, m: pick(batch.support_batch(A, b, SUPPORT_C, m=m), ("h", "x", "status")),
                                bounded(16, 3, 41), bounded(16, 3, 42)),
        "py-subset": G(lambda A, b, m, QA, Qb, mq: dict(sub=batch.subset_batch(A, b, QA, Qb, m=m, mq=mq)),
                       subset_case(45, 0), subset_case(46, 1), differ=("sub",), ref=ref_subset),
        "py-hull-fmax": G(lambda X, n: pick(batch.hull_batch(X, n=n), ("A", "b", "on", "count", "status")), points_case(47),
                          points_case(48)),
    }


NAMES = ["lp-n3-phase1", "lp-n8", "cheby-dup", "bbox-dup", "reduce-second-pass", "reduce-wide-70", "contains-per-polytope",
         "contains-region", "pairs", "fm", "volume-hits", "support", "extreme", "hull", "vol-exact", "assign-F9", "assign-F600",
         "hull-reassign", "locate-grid", "py-projection", "py-extreme-reduce", "py-volume-exact-reduce", "py-volume-own-boxes",
         "py-support-resolve", "py-subset", "py-hull-fmax"]
CONTROLS = ["contains-per-polytope", "cheby-dup", "py-extreme-reduce"]


# ------------------------------------------------------------------------------------------------ the delay
class Delay:
    """A stretch of device time on the current stream: torch.cuda._sleep where present, else a chain of matmuls; sized once
    with events (ms per unit), enqueued in pieces of at most 50 ms."""

    def __init__(self, torch):
        self.torch, self.ms = torch, 0.0
        self.sleep = getattr(torch.cuda, "_sleep", None)
        self.x = None if self.sleep else torch.randn(2048, 2048, device="cuda:0")
        self.unit = 2_000_000 if self.sleep else 4   # cycles, or matmuls
        for _ in range(2):   # (the second measurement: the first pays for loading the kernel)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            self._units(1)
            e1.record()
            e1.synchronize()
            self.unit_ms = max(e0.elapsed_time(e1), 1e-3)

    def _units(self, n):
        if self.sleep:
            self.sleep(int(n * self.unit))
        else:
            for _ in range(int(n * self.unit)):
                self.x = (self.x @ self.x).clamp_(-1.0, 1.0)

    def __call__(self):
        left = self.ms
        while left > 0:
            piece = min(left, 50.0)
            self._units(max(1, int(np.ceil(piece / self.unit_ms))))
            left -= piece


class Prepared:
    pass


@pytest.fixture(scope="module")
def P(tmp_path_factory, reduce_plan):
    """The cases on the device, their synchronised answers for both batches (which is also the warm-up), the time of the
    slowest gated call -- default stream, device idle, from the first enqueue to completion with the host's share -- and
    the delay: ten times that (a busy shared machine), at least 20 ms (the Python layer's launch path)."""
    import torch
    P = Prepared()
    P.torch = torch
    P.cases = build_cases()
    assert list(P.cases) == NAMES
    got = dict(zip(FIELDS, reduce_plan(B, 16, 3, {k[len("PLP_REDUCE_"):]: str(v) for k, v in SECOND_PASS.items()})))
    assert got["second"] == 1 and got["force_retry"] == 1, got
    P.real_t, P.decoy_t, P.want, P.want_decoy, P.ms = {}, {}, {}, {}, {}
    for name, c in P.cases.items():
        if c.prepare:
            c.prepare(c)
        P.real_t[name], P.decoy_t[name] = c.tensors(c.real), c.tensors(c.decoy)
        with switches(c.env):
            for args, out in ((P.decoy_t[name], P.want_decoy), (P.real_t[name], P.want)):
                res = c.fn(**args)
                torch.cuda.synchronize()
                out[name] = host(res)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            c.fn(**P.real_t[name])
            torch.cuda.synchronize()
            P.ms[name] = 1e3 * (time.perf_counter() - t0)
    P.delay = Delay(torch)
    P.probe = torch.zeros(1, device="cuda:0")
    P.slowest = max(P.ms, key=P.ms.get)
    P.delay.ms = max(20.0, 10.0 * P.ms[P.slowest])
    print("\nstreams: slowest gated call %s %.2f ms (median of the cases %.2f ms); gate delay %.1f ms (%s, %.3f ms per unit)" % (
        P.slowest, P.ms[P.slowest], float(np.median(list(P.ms.values()))), P.delay.ms,
        "torch.cuda._sleep" if P.delay.sleep else "matmuls", P.delay.unit_ms))
    return P


@pytest.fixture(scope="module")
def R(oracle, tmp_path_factory):
    """The outside references: the oracle and the host builds of the enumeration kernels (compiled side by side)."""
    R = Prepared()
    R.O = oracle
    tmp = tmp_path_factory.mktemp("streams_host")
    with concurrent.futures.ThreadPoolExecutor(3) as pool:
        jobs = [pool.submit(mod.build, tmp) for mod in (xh, hh, vh)]
        R.xh, R.hh, R.vh = [j.result() for j in jobs]
    return R


# ------------------------------------------------------------------------------------------------ 1: the gate
def fresh_inputs(P, name):
    """The case's input tensors holding the decoy (fresh copies; the device is idle when this returns)."""
    live = {k: (v.clone() if hasattr(v, "clone") else v) for k, v in P.decoy_t[name].items()}
    P.torch.cuda.synchronize()
    return live


def refill(live, real):
    for k, v in live.items():
        if hasattr(v, "copy_"):
            v.copy_(real[k])


def runs_apart(P, busy, other):
    """Does work on the stream `other` run while `busy` is busy?  The runtime maps the streams of a process onto a few
    hardware queues (four unless told otherwise) and two streams that share one run in order: a launch that went to
    `other` by mistake would then wait for the gate like the rest and go unseen.  Probe: the delay on `busy`, a one-element
    fill on `other`, which must have finished while the delay is still running."""
    torch = P.torch
    behind = torch.cuda.Event()
    with torch.cuda.stream(busy):
        P.delay()
        behind.record(busy)
    with torch.cuda.stream(other):
        P.probe.fill_(1.0)
    other.synchronize()
    apart = not behind.query()
    busy.synchronize()
    return apart


def stream_apart_from(P, other, busy_is_new=True, tries=12):
    """A pool stream that runs side by side with `other` (busy_is_new: the new stream carries the delay in the probe)."""
    for _ in range(tries):
        s = P.torch.cuda.Stream()
        if s.cuda_stream != other.cuda_stream and (runs_apart(P, s, other) if busy_is_new else runs_apart(P, other, s)):
            return s
    pytest.fail("none of %d streams runs side by side with stream %#x: nothing can be told apart by timing here" % (tries, other.cuda_stream))


def two_streams(P):
    """Two pool streams that run side by side with each other, the first also with the default stream (where the tests
    read results back)."""
    s = stream_apart_from(P, P.torch.cuda.default_stream())
    return s, stream_apart_from(P, s, busy_is_new=False)


@pytest.mark.parametrize("name", NAMES)
def test_decoy_answer_differs(P, name):
    """Both batches are valid and their answers differ: an answer for the decoy cannot pass as the real one."""
    c, x, y = P.cases[name], P.want[name], P.want_decoy[name]
    if c.differ == "members":
        d = members_differ(x, y)
        assert d is not None and d.all(), (name, np.nonzero(~d)[0][:8].tolist())
    else:
        for key in c.differ:
            assert share_differs(x, y, key) >= 0.25, (name, key, share_differs(x, y, key))


@pytest.mark.parametrize("name", NAMES)
def test_call_waits_for_its_own_stream(P, name):
    torch, c = P.torch, P.cases[name]
    live = fresh_inputs(P, name)
    s = stream_apart_from(P, torch.cuda.default_stream())   # (what lands on the NULL stream does not queue behind the gate)
    with switches(c.env), torch.cuda.stream(s):
        P.delay()
        refill(live, P.real_t[name])
        res = c.fn(**live)
        clones = {k: v.clone() for k, v in res.items() if v is not None}
    s.synchronize()
    assert_same(host(clones), P.want[name], (name, "gated on its stream"))


@pytest.mark.parametrize("name", CONTROLS)
def test_control_call_on_another_stream_sees_the_decoy(P, name):
    """The detector's power: the same sequence with the call misplaced on a second stream answers for the decoy, and the
    gate on the first stream is still closed once that answer has been read back."""
    torch, c = P.torch, P.cases[name]
    live = fresh_inputs(P, name)
    s, s2 = two_streams(P)
    opened = torch.cuda.Event()
    with torch.cuda.stream(s):
        P.delay()
        refill(live, P.real_t[name])
        opened.record(s)
    t0 = time.perf_counter()
    with switches(c.env), torch.cuda.stream(s2):
        res = c.fn(**live)
        clones = {k: v.clone() for k, v in res.items() if v is not None}
    s2.synchronize()
    got = host(clones)
    pending = not opened.query()
    took = 1e3 * (time.perf_counter() - t0)
    s.synchronize()
    assert pending, ("delay too short: the copy on the first stream had run by the time the misplaced call was read back "
                     "(%.2f ms; the call alone took %.2f ms, the delay is %.1f ms)" % (took, P.ms[name], P.delay.ms))
    assert_same(got, P.want_decoy[name], (name, "misplaced on a second stream"))


# ------------------------------------------------------------------------------------------------ 6: the outside reference
@pytest.mark.parametrize("name", [n for n in NAMES])
def test_synchronised_answer_against_the_outside_reference(P, R, name):
    c = P.cases[name]
    if c.ref is None:
        assert name in ("fm", "volume-hits") or name.startswith("py-")   # (the module docstring says why)
        return
    c.ref(P.want[name], c.real, R)


# ------------------------------------------------------------------------------------------------ 2: per-stream scratch
SIZES_A = (64, 2000, 64, 5000, 64, 2000, 64, 5000)
SIZES_B = (2000, 64, 5000, 64, 2000, 64, 5000, 64)   # out of step: a buffer grows while the other stream is busy


def lp_family_calls(torch, fam, n, seed):
    """The three verified calls on one batch of a family, the last one cheby_ball_batch -> [(name, fn of no argument)]."""
    a = {k: to_dev(v) for k, v in (dup(seed, n) if fam == "dup" else unbounded(seed, n)).items()}
    c = to_dev(np.random.default_rng(seed + 1).standard_normal((n, 3)))
    return [("bbox " + fam, lambda: batch.bbox_batch(a["A"], a["b"], a["m"])),
            ("lpsolve " + fam, lambda: batch.lpsolve_batch(c, a["A"], a["b"], a["m"])),
            ("cheby " + fam, lambda: batch.cheby_ball_batch(a["A"], a["b"], a["m"]))]


def test_verifier_scratch_of_two_streams(P):
    """Eight rounds, no host synchronisation inside a round: on each stream bbox, lpsolve and cheby_ball on a `dup` and then
    on an `unbounded` batch, the two streams taking turns call by call; the batch sizes go 64 -> 2000 -> 64 -> 5000 on one
    stream and out of step on the other.  Bit for bit the synchronised single-stream results; after every round the
    careful count of each stream is what its last call (cheby_ball_batch, unbounded: every unbounded member is on the
    list) reports when run alone."""
    torch = P.torch
    calls, want, alone, counts = {}, {}, {}, {}
    for n in (64, 2000, 5000):
        calls[n] = lp_family_calls(torch, "dup", n, 100 + n) + lp_family_calls(torch, "unbounded", n, 200 + n)
        want[n], counts[n] = [], []
        for _, fn in calls[n]:
            res = fn()
            torch.cuda.synchronize()
            want[n].append(host(res))
            counts[n].append(batch.verify_careful_lps())   # (the default stream)
        alone[n] = counts[n][-1]
        assert alone[n] > 0, (n, counts[n])
    sa, sb = two_streams(P)
    torch.cuda.synchronize()
    seen, results = [], []
    for rnd, (na, nb) in enumerate(zip(SIZES_A, SIZES_B)):
        for k in range(6):
            for s, n in ((sa, na), (sb, nb)):
                with torch.cuda.stream(s):
                    results.append((rnd, n, k, calls[n][k][1]()))
        # (the query blocks on its own stream only, between two rounds)
        ca, cb = batch.verify_careful_lps(stream=sa), batch.verify_careful_lps(stream=sb)
        seen.append((ca, cb))
        assert ca == alone[na] and cb == alone[nb], (rnd, ca, alone[na], cb, alone[nb])
    sa.synchronize()
    sb.synchronize()
    for rnd, n, k, res in results:
        assert_same(host(res), want[n][k], ("round", rnd, "B", n, calls[n][k][0]))
    assert batch.verify_careful_lps(stream=sa) > 0 and batch.verify_careful_lps(stream=sb) > 0
    print("\nstreams: verify_careful_lps after %s alone, by batch size: %s; per round (stream A, stream B): %s" % (
        [name for name, _ in calls[64]], counts, seen))


def test_assign_scratch_of_two_streams(P):
    """assign_batch at F = 9 (the per-stream partials of plp_assign_dev), N = 5000 and N = 200 000 out of step."""
    torch = P.torch
    data, want = {}, {}
    for n in (5000, 200000):
        data[n] = [to_dev(v) for v in quickhull_workload(n, d=3, F=9, seed=n)]
        res = batch.assign_batch(*data[n])
        torch.cuda.synchronize()
        want[n] = host(res)
    sa, sb = two_streams(P)
    torch.cuda.synchronize()
    results = []
    for na, nb in ((5000, 200000), (200000, 5000)) * 2:
        for s, n in ((sa, na), (sb, nb)):
            with torch.cuda.stream(s):
                results.append((n, batch.assign_batch(*data[n])))
    sa.synchronize()
    sb.synchronize()
    for n, res in results:
        assert_same(host(res), want[n], ("assign", n))


# ------------------------------------------------------------------------------------------------ 3: the 17th stream
def test_twenty_streams(P):
    """cheby_ball (dup), bbox and an F = 9 assign on twenty streams and again in reverse order: the tables of 16 are emptied
    (after a device synchronisation) when the 17th stream shows up, twice."""
    torch = P.torch
    a = {k: to_dev(v) for k, v in dup(300, 64).items()}
    pts = [to_dev(v) for v in quickhull_workload(NPTS, d=3, F=9, seed=300)]
    fns = [lambda: batch.cheby_ball_batch(a["A"], a["b"], a["m"]), lambda: batch.bbox_batch(a["A"], a["b"], a["m"]),
           lambda: batch.assign_batch(*pts)]
    want = []
    for fn in fns:
        res = fn()
        torch.cuda.synchronize()
        want.append(host(res))
    streams = [torch.cuda.Stream() for _ in range(20)]
    assert len({s.cuda_stream for s in streams}) == 20
    results = []
    for s in streams + streams[::-1]:
        with torch.cuda.stream(s):
            results += [(k, fn()) for k, fn in enumerate(fns)]
    torch.cuda.synchronize()
    for k, res in results:
        assert_same(host(res), want[k], ("twenty streams", k))
    left = batch.verify_careful_lps(stream=streams[0])   # (0 when its entry went with the table)
    assert isinstance(left, int) and left >= 0


# ------------------------------------------------------------------------------------------------ 4: the ring of 64
@pytest.mark.parametrize("env", [{"PLP_REDUCE_RETRY_ALL": 1}, SECOND_PASS], ids=["retry-all", "retry-all-second-pass"])
def test_eighty_reduces_in_flight(P, reduce_plan, env):
    """80 reduce_batch calls of 33 members of (16, 3) on two streams in turn, two batches in turn, nothing synchronised
    until the end: call e and call e + 64 share a retry word.  Then once more with the simplex counter switched on from
    the second stream: it ends at the sum of the 80 calls' own counts (each batch's measured alone).
    retry-all is the environment as the issue names it (at this shape the lane kernel: complete in one launch);
    retry-all-second-pass the engine that raises the retry words and is followed by the second pass."""
    torch = P.torch
    second = dict(zip(FIELDS, reduce_plan(33, 16, 3, {k[len("PLP_REDUCE_"):]: str(v) for k, v in env.items()})))["second"]
    assert second == (1 if env is SECOND_PASS else 0)
    data = [{k: to_dev(v) for k, v in bounded(16, 3, 400 + i, n=33).items()} for i in range(2)]
    s1, s2 = two_streams(P)
    with switches(env):
        want = []
        for a in data:
            res = batch.reduce_batch(a["A"], a["b"], a["m"])
            torch.cuda.synchronize()
            want.append(host(res))

        def eighty():
            out = []
            for e in range(80):
                with torch.cuda.stream((s1, s2)[e % 2]):
                    out.append(batch.reduce_batch(**data[(e // 2) % 2]))
            torch.cuda.synchronize()
            return out
        for e, res in enumerate(eighty()):
            assert_same(host(res), want[(e // 2) % 2], ("reduce in flight", e))
        batch.reduce_simplex_runs(reset=True, stream=s2)
        own = []
        for a in data:
            batch.reduce_batch(a["A"], a["b"], a["m"])
            torch.cuda.synchronize()
            own.append(batch.reduce_simplex_runs(reset=True, stream=s2))
        assert min(own) > 0, own
        for e, res in enumerate(eighty()):
            assert_same(host(res), want[(e // 2) % 2], ("reduce in flight, counting", e))
        assert batch.reduce_simplex_runs(reset=True, stream=s2) == 40 * (own[0] + own[1]), own


# ------------------------------------------------------------------------------------------------ 5: contains across streams
def test_contains_across_streams(P, oracle):
    """Tables of P = 40 and P = 300 polytopes of (16, 4) on two streams in turn, eight rounds with both in flight; then a
    table of P = 3000 from the second stream -- the thresholds buffer grows -- while the first stream's call is queued
    behind a delay.  Whether two calls overlap is a matter of timing: a missing hand-over shows here only when they do."""
    torch = P.torch
    X = np.random.default_rng(500).uniform(-1.5, 1.5, (4, NPTS))
    Xt = to_dev(X)
    tabs, want = {}, {}
    for n in (40, 300, 3000):
        a = bounded(16, 4, 500 + n, n=n)
        tabs[n] = (a, {k: to_dev(v) for k, v in a.items()})
        res = batch.contains_batch(tabs[n][1]["A"], tabs[n][1]["b"], Xt, m=tabs[n][1]["m"], region=False)
        torch.cuda.synchronize()
        want[n] = res.cpu().numpy()
    a40 = tabs[40][0]
    ref = np.stack([oracle.contains(a40["A"][p:p + 1, :a40["m"][p]], a40["b"][p:p + 1, :a40["m"][p]],
                                    np.ascontiguousarray(X[:, :200].T))[0] for p in range(40)])
    assert np.array_equal(want[40][:, :200], ref) and 0 < ref.sum() < ref.size

    def call(n):
        t = tabs[n][1]
        return n, batch.contains_batch(t["A"], t["b"], Xt, m=t["m"], region=False)
    s1, s2 = two_streams(P)
    torch.cuda.synchronize()
    results = []
    for rnd in range(8):
        for s, n in ((s1, 40), (s2, 300)) if rnd % 2 == 0 else ((s1, 300), (s2, 40)):
            with torch.cuda.stream(s):
                results.append(call(n))
    with torch.cuda.stream(s1):
        P.delay()
        results.append(call(300))
    with torch.cuda.stream(s2):
        results.append(call(3000))
        results.append(call(40))
    with torch.cuda.stream(s1):
        results.append(call(40))
    s1.synchronize()
    s2.synchronize()
    for n, res in results:
        assert np.array_equal(res.cpu().numpy(), want[n]), ("contains across streams", n)
