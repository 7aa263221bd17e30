"""GPU: projection_hull_batch (projhull_kernel, one polytope per wavefront) and projection_batch(solver="iterhull") -- every
case of g31 through the raw call (numpy and CUDA tensors) under the three checks that define "correct" and against the host
rule, random shapes over every kernel instance and both sides of each padding step at B = 1, 5 and 257 with ragged m, an
unbounded and a flat member, poison in everything the kernel must not read, the public call against Fourier-Motzkin, the
overflow cases through the single call, and the caller's stream."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import projhull_host as PH  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    from polytope_amd import solvers
    old, solvers.default_solver = solvers.default_solver, "hip"
    yield
    solvers.default_solver = old


@pytest.fixture(scope="module")
def cases():
    return PH.load()


@pytest.fixture(scope="module")
def groups(cases):
    """The fixture's cases grouped by (d, dim): one packed batch each, NaN beyond m."""
    out = {}
    for c in cases:
        out.setdefault((c.A.shape[1], tuple(int(v) for v in c.dim)), []).append(c)
    return [(dim, cs) + PH.pack([(c.A, c.b) for c in cs]) for (_, dim), cs in sorted(out.items())]


def _host(res):
    return {k: (v.cpu().numpy().view(np.uint64) if k in ("on", "vmask") else v.cpu().numpy()) for k, v in res.items()}


def _lp_support(A, b, m, owner, C):
    """max C[t] . x over polytope owner[t], all through ONE certified lpsolve_batch -> h[T]."""
    from polytope_amd import batch
    A3 = np.nan_to_num(A[owner])
    out = batch.lpsolve_batch(-C, A3, np.nan_to_num(b[owner]), m=m[owner].astype(np.int32))
    assert not out["status"].any()
    return -out["fun"]


@pytest.mark.parametrize("tensors", [False, True])
def test_fixture_cases(groups, tensors, tmp_path_factory):
    """Every fixture case through the raw call: the expected status, (a), (b), (c), and the status and (on pinned cases)
    the row count of the host rule with the oracle's LPs.  No bitwise claim: the LP engines differ."""
    from polytope_amd import batch
    L = PH.build(tmp_path_factory.mktemp("projhull_host"))
    worst_outer, worst_ref = -np.inf, -np.inf
    for dim, cs, A, b, m in groups:
        if tensors:
            import torch
            res = _host(batch.projection_hull_batch(*[torch.as_tensor(a, device="cuda:0") for a in (A, b)], list(dim),
                                                    m=torch.as_tensor(m, device="cuda:0"), points=True))
        else:
            res = batch.projection_hull_batch(A, b, list(dim), m=m, points=True)
        for p, c in enumerate(cs):
            assert int(res["status"][p]) == c.expect, (c.index, c.family, int(res["status"][p]))
            assert int(res["nlp"][p]) >= int(res["m"][p])
            lp = PH.oracle_lp(c.A, c.b)
            host = PH.run(L, c.A[None], c.b[None], None, c.dim, PH.centre(c.A, c.b)[None], lambda _p, cc: lp(cc))
            assert int(host["status"][0]) == int(res["status"][p])
            if c.expect != PH.PH_OK:
                assert int(res["m"][p]) == 0 and np.all(np.isnan(res["A"][p]))
                continue
            if c.pinned:
                assert int(host["m"][0]) == int(res["m"][p]), (c.index, c.family)
            outer, ref = PH.check_all(c, res, p)
            worst_outer = max(worst_outer, outer)
            worst_ref = max(worst_ref, ref if c.pinned else -np.inf)
    print("projhull gpu: worst outer excess %.3g, worst excess over ref_gap %.3g (units of the frame)" % (worst_outer, worst_ref))


# (m, d, k): the issue's shapes, then d = 9, 12, 13 -- with d = 4 | 5, 8 | 9, 12 | 13 both sides of every padding step of
# the instances D = 4, 8, 12, 16
SHAPES = [(6, 3, 1), (7, 3, 2), (9, 4, 2), (12, 5, 2), (14, 5, 3), (20, 6, 2), (28, 8, 2), (32, 6, 3), (64, 16, 2),
          (24, 9, 2), (30, 12, 2), (32, 13, 3)]


def _random_batch(rng, B, m, d, k):
    """B polytopes: the box |x| <= 1 and m - 2 d random cuts at radius 0.5 .. 0.9 (k = 3: 1.0 .. 1.6, which keeps the
    projections of all the shapes below within 64 points: the host rule holds at most 32), up to three trailing cuts
    dropped per member (ragged m), NaN beyond m; from B = 5 on member 1 is unbounded along the first kept coordinate and (k >= 2) member 3
    is 1e-10 thin along it.  -> A, b, mrows, dim, expect."""
    dim = np.sort(rng.choice(d, k, replace=False)) + 1
    A, b = np.full((B, m, d), np.nan), np.full((B, m), np.nan)
    mrows, expect = np.zeros(B, np.int32), np.zeros(B, np.int32)
    j = int(dim[0]) - 1
    for p in range(B):
        cuts = m - 2 * d
        R = rng.standard_normal((cuts, d))
        R /= np.linalg.norm(R, axis=1)[:, None]
        a = np.vstack([np.eye(d), -np.eye(d), R])
        bb = np.concatenate([np.ones(2 * d), rng.uniform(*((0.5, 0.9) if k < 3 else (1.0, 1.6)), cuts)])
        mp = m - int(rng.integers(0, min(3, cuts) + 1))
        if B >= 5 and p == 1:
            a[:, j] = np.minimum(a[:, j], 0.0)
            a[j], bb[j] = a[d + j], bb[d + j]   # (the row x_j <= 1 became a zero row: -x_j <= 1 twice)
            expect[p] = PH.PH_UNBOUNDED
        if B >= 5 and p == 3 and k >= 2:
            bb[j], bb[d + j] = 0.25 + 1e-10, -0.25 + 1e-10
            a[2 * d:, j] = 0.0   # (the cuts do not look at x_j: the slab keeps its centre)
            expect[p] = PH.PH_FLAT
        A[p, :mp], b[p, :mp], mrows[p] = a[:mp], bb[:mp], mp
    return A, b, mrows, dim, expect


@pytest.mark.parametrize("B", [1, 5, 257])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d-%d" % s)
def test_random_shapes(shape, B):
    """Statuses, (a) with the certified lpsolve_batch as the independent LP, and (b), on ragged batches."""
    from polytope_amd import batch
    m, d, k = shape
    rng = np.random.default_rng(1000 * m + 10 * d + k + B)
    A, b, mrows, dim, expect = _random_batch(rng, B, m, d, k)
    res = batch.projection_hull_batch(A, b, list(dim), m=mrows, points=True)
    assert np.array_equal(res["status"], expect), (res["status"], expect)
    ok = np.nonzero(expect == PH.PH_OK)[0]
    cnt, nv = res["m"], res["nv"]
    assert np.all(res["nlp"][ok] >= cnt[ok]) and np.all(cnt[ok] >= (2 if k == 1 else k + 1)) and not cnt[expect != 0].any()
    owner = np.repeat(ok, cnt[ok])
    rows = np.concatenate([res["A"][p, :cnt[p]] for p in ok])
    rhs = np.concatenate([res["b"][p, :cnt[p]] for p in ok])
    assert np.all(np.abs(np.linalg.norm(rows, axis=1) - 1.0) <= 1e-12)
    Cs = np.zeros((owner.size, d))
    Cs[:, dim - 1] = rows
    h = _lp_support(A, b, mrows, owner, Cs)
    scale = np.array([PH.scale_of(res["V"][p, :nv[p]]) if nv[p] else 1.0 for p in range(B)])
    excess = (h - rhs) / scale[owner]
    print("projhull gpu %s B=%d: worst outer excess %.3g, LPs per polytope %.1f" % (shape, B, excess.max(), res["nlp"][ok].mean()))
    assert np.all(excess <= 2 * PH.CONF_TOL)
    for p in ok:
        PH.check_inner(A[p, :mrows[p]], b[p, :mrows[p]], dim, res["V"][p, :nv[p]], res["X"][p, :nv[p]])
        assert np.all(np.isnan(res["A"][p, cnt[p]:])) and np.all(np.isnan(res["V"][p, nv[p]:])) and not res["on"][p, cnt[p]:].any()


def test_poison_and_empty_members():
    """Rows beyond m[p] hold NaN; whole members with m[p] = 0 (all NaN) stand between the others: those get PH_NOCENTRE,
    and the others' outputs are the bits of the batch without them."""
    from polytope_amd import batch
    rng = np.random.default_rng(77)
    A, b, mrows, dim, expect = _random_batch(rng, 7, 14, 5, 2)
    want = batch.projection_hull_batch(A, b, list(dim), m=mrows, points=True)
    where = np.array([1, 2, 4, 5, 7, 8, 9])
    A2, b2, m2 = np.full((11, 14, 5), np.nan), np.full((11, 14), np.nan), np.zeros(11, np.int32)
    A2[where], b2[where], m2[where] = A, b, mrows
    got = batch.projection_hull_batch(A2, b2, list(dim), m=m2, points=True)
    rest = np.setdiff1d(np.arange(11), where)
    assert np.all(got["status"][rest] == PH.PH_NOCENTRE) and not got["m"][rest].any() and not got["nlp"][rest].any()
    for key in want:
        assert np.array_equal(got[key][where], want[key], equal_nan=True), key


def _vertices(A, b):
    from polytope_amd import polytope as pc
    return np.asarray(pc.extreme(pc.Polytope(A, b, normalize=False)))


def test_public_call_against_fourier_motzkin(hip):
    """projection_batch(solver="iterhull") and (solver="fm") on 40 horizon polytopes at (n, k, N) = (2, 1, 2) give the same
    polytopes: the vertices of each satisfy the rows of the other to 1e-7 of their extent (the reduce tolerance of both
    paths).  solver="fm" and no solver: the same bits.  solver=None: fm here (two deleted coordinates), the hull at N = 3."""
    from polytope_amd import batch, synth
    A, b = synth.horizon_polytopes(40, 2, 1, 2, 6, seed=5)
    fm = batch.projection_batch(A, b, [1, 2], solver="fm")
    plain = batch.projection_batch(A, b, [1, 2])
    hull = batch.projection_batch(A, b, [1, 2], solver="iterhull")
    auto = batch.projection_batch(A, b, [1, 2], solver=None)
    assert sorted(fm) == sorted(plain) == sorted(hull) == sorted(auto)
    for key in fm:
        assert np.array_equal(fm[key], plain[key]) and np.array_equal(fm[key], auto[key]), key
    assert not fm["status"].any() and not hull["status"].any() and hull["routed"] == 0
    for p in range(40):
        Pf = (fm["A"][p, :fm["m"][p]], fm["b"][p, :fm["m"][p]])
        Ph = (hull["A"][p, :hull["m"][p]], hull["b"][p, :hull["m"][p]])
        Vf, Vh = _vertices(*Pf), _vertices(*Ph)
        tol = 1e-7 * max(1.0, PH.scale_of(Vf))
        assert Vf.shape[0] >= 3 and Vh.shape[0] >= 3
        assert np.max(Vf @ Ph[0].T - Ph[1][None, :]) <= tol and np.max(Vh @ Pf[0].T - Pf[1][None, :]) <= tol, p
    A3, b3 = synth.horizon_polytopes(6, 2, 1, 3, 6, seed=6)
    auto3, hull3 = batch.projection_batch(A3, b3, [1, 2], solver=None), batch.projection_batch(A3, b3, [1, 2], solver="iterhull")
    for key in hull3:
        assert np.array_equal(auto3[key], hull3[key]), key
    assert not hull3["status"].any()
    with pytest.raises(ValueError):
        batch.projection_batch(A, b, [1, 2], solver="exthull")


def test_overflow_cases_are_routed(hip, cases):
    """The two cases of more than 64 vertices come back through the single call: routed, status 0, and the reference's
    polytope (its vertices hold our rows, our vertices hold its rows, to the 1e-7 both iterhulls stop at)."""
    from polytope_amd import batch
    over = [c for c in cases if c.expect == PH.PH_OVERFLOW_POINTS]
    assert len(over) == 2
    A, b, m = PH.pack([(c.A, c.b) for c in over])
    np.random.seed(0)
    res = batch.projection_batch(np.nan_to_num(A), np.nan_to_num(b), list(over[0].dim), m=m, solver="iterhull")
    assert res["routed"] == 2 and not res["status"].any()
    for p, c in enumerate(over):
        Ao, bo = res["A"][p, :res["m"][p]], res["b"][p, :res["m"][p]]
        s = PH.scale_of(c.ref_V)
        assert np.max(c.ref_V @ Ao.T - bo[None, :]) <= 1e-7 * s + c.ref_gap
        PH.check_outer(c.A, c.b, c.dim, Ao / np.linalg.norm(Ao, axis=1)[:, None], bo / np.linalg.norm(Ao, axis=1) + 1e-7 * s, s)


def test_the_call_runs_on_the_callers_stream():
    """CUDA tensors in, on a stream of its own.  The tensors hold a decoy batch; on the stream: a delay, the copy of the
    real batch into the tensors, the call, clones of the outputs; only that stream is synchronised.  The rows are the real
    batch's -- a launch that went to the default stream would have answered for the decoy."""
    import torch
    from polytope_amd import batch
    import test_streams_gpu as TSG
    rng = np.random.default_rng(9)
    A, b, mrows, dim, _ = _random_batch(rng, 4, 14, 5, 2)
    A, b = np.nan_to_num(A), np.nan_to_num(b)
    decoy_b = b * 0.5
    xc = np.zeros((4, 5))   # (strictly inside both; given, so that the call is the one launch)
    want, other = (batch.projection_hull_batch(A, bb, list(dim), m=mrows, xc=xc) for bb in (b, decoy_b))
    assert not np.array_equal(want["b"], other["b"], equal_nan=True)
    live = [torch.as_tensor(a, device="cuda:0") for a in (A, decoy_b)]
    mt, xt, src_b = (torch.as_tensor(a, device="cuda:0") for a in (mrows, xc, b))
    warm = batch.projection_hull_batch(live[0], live[1], list(dim), m=mt, xc=xt)
    torch.cuda.synchronize()
    assert np.array_equal(warm["b"].cpu().numpy(), other["b"], equal_nan=True)
    P = TSG.Prepared()
    P.torch, P.delay, P.probe = torch, TSG.Delay(torch), torch.zeros(1, device="cuda:0")
    P.delay.ms = 20.0
    s = TSG.stream_apart_from(P, torch.cuda.default_stream())
    with torch.cuda.stream(s):
        P.delay()
        live[1].copy_(src_b)
        res = batch.projection_hull_batch(live[0], live[1], list(dim), m=mt, xc=xt)
        clones = {k: v.clone() for k, v in res.items()}
    s.synchronize()
    assert all(v.is_cuda for v in res.values())
    got = _host(clones)
    for key in want:
        assert np.array_equal(got[key], want[key], equal_nan=True), key
