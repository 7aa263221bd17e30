"""GPU: support_kernel (csrc/plp_support.hip) through batch.support_batch / subset_batch and the C ABI, against the host
build of the same source (tests/cabi/support_host.cpp: statuses identical, h bit for bit) and against the oracle's simplex.

Tolerance against the oracle (tests/support_host.py: check_against_oracle): status equal to oracle.lp_solve's; where it is
0, |h - (-fun)| <= 1e-9 max(1, |h|); x is not compared (ties have no unique vertex) but A x <= b + 1e-9 and
|c.x - h| <= 1e-12 max(1, |h|)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from polytope_amd import _lib, batch  # noqa: E402
from polytope_amd.synth import random_hpolytopes  # noqa: E402
import support_host as sh  # noqa: E402
from test_support_host import family_case, soak_family_case  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def L(tmp_path_factory):
    return sh.build(tmp_path_factory.mktemp("support_host"))


def dev(*arrays):
    import torch
    return [None if a is None else torch.as_tensor(a).to("cuda:0") for a in arrays]


def same_bits(a, b):
    return np.array_equal(np.asarray(a).view(np.int64), np.asarray(b).view(np.int64))


def ragged(B, m_max, d, seed):
    A, b = random_hpolytopes(B, m_max, d, seed=seed)
    m = np.random.default_rng(seed + 1).integers(2 * d, m_max + 1, size=B).astype(np.int32)
    m[0] = m_max
    for p in range(B):
        A[p, m[p]:] = 0.0
        b[p, m[p]:] = 0.0
    return A, b, m


# ------------------------------------------------------------------------------------------ raw answers: the host build
@pytest.mark.parametrize("m_max", [16, 17, 33, 64])
@pytest.mark.parametrize("d", [1, 2, 3, 4])
def test_raw_answers_equal_the_host_build(L, d, m_max):
    """resolve=False against the host build: B in {1, 5, 257} (257 crosses a workgroup's polytope count for every tile),
    K in {1, 3, 64, 65, 130} (the lanes-per-polytope steps and the round loop), every row-slot count with zero-row padding,
    d = 1..4, both layouts of C.  Statuses identical, h bit for bit where the status is 0, x likewise; torch tensors in
    give the numpy call's bits."""
    rng = np.random.default_rng(1000 * d + m_max)
    for B in (1, 5, 257):
        A, b, m = ragged(B, m_max, d, seed=31 * d + m_max + B)
        xc = batch.cheby_ball_batch(A, b, m)["xc"]
        for K in (1, 3, 64, 65, 130):
            shared = (K + B) % 2 == 0
            C_ = rng.standard_normal((K, d) if shared else (B, K, d))
            want_h, want_x, want_st = sh.run(L, A, b, C_, xc, m)
            res = batch.support_batch(A, b, C_, m=m, xc=xc, resolve=False)
            assert np.array_equal(res["status"], want_st), (B, K, np.argwhere(res["status"] != want_st)[:5])
            ok = want_st == 0
            assert ok.mean() > 0.98
            assert same_bits(res["h"][ok], want_h[ok]), (B, K)
            assert same_bits(res["x"][ok], want_x[ok]), (B, K)
            assert np.all(np.isnan(res["h"][want_st == 1]))
            if B == 257 or K == 65:
                At, bt, mt, Ct, xt = dev(A, b, m, C_, xc)
                rt = batch.support_batch(At, bt, Ct, m=mt, xc=xt, resolve=False)
                assert rt["h"].is_cuda and np.array_equal(rt["status"].cpu().numpy(), res["status"])
                assert np.array_equal(rt["h"].cpu().numpy(), res["h"], equal_nan=True)
                assert np.array_equal(rt["x"].cpu().numpy(), res["x"], equal_nan=True)


# ------------------------------------------------------------------------------------------ the families of the CPU test
@pytest.mark.parametrize("shared", [True, False])
@pytest.mark.parametrize("k", range(len(sh.SHAPES)))
def test_families_raw_and_resolved(L, oracle, k, shared):
    """The families and seeds of tests/test_support_host.py: raw answers equal the host build's (so the hand-back share
    is the host's, under the same 1 % cap); resolved answers equal the oracle's, numpy and torch inputs, with the
    centre given and with the centre left to cheby_ball_batch."""
    A, b, m, C_, xc, ost, oh = family_case(oracle, k, shared)
    want_h, _, want_st = sh.run(L, A, b, C_, xc, m)
    raw = batch.support_batch(A, b, C_, m=m, xc=xc, resolve=False)
    assert np.array_equal(raw["status"], want_st)
    assert same_bits(raw["h"][want_st == 0], want_h[want_st == 0])
    assert (raw["status"] == 1).sum() == (want_st == 1).sum() <= sh.HANDBACK_CAP * want_st.size
    for centre in (xc, None):
        res = batch.support_batch(A, b, C_, m=m, xc=centre)
        sh.check_against_oracle(A, b, m, C_, res["h"], res["x"], res["status"], ost, oh)
    At, bt, mt, Ct = dev(A, b, m, C_)
    rt = batch.support_batch(At, bt, Ct, m=mt)
    sh.check_against_oracle(A, b, m, C_, rt["h"].cpu().numpy(), rt["x"].cpu().numpy(), rt["status"].cpu().numpy(), ost, oh)


ALL_FAMILIES = sh.FAMILIES + ("degenerate",)


@pytest.mark.parametrize("fam", ALL_FAMILIES)
def test_soak_families_raw_equal_the_host_build(L, oracle, fam):
    """The inputs of tests/test_support_host.py: test_soak_families_equal_the_oracle / test_degenerate_vertices_equal_the_oracle
    (the seven soak families, NaN centres included, both layouts of C; `dup` also on the stream of seed 8): statuses
    identical to the host build's, h and x bit for bit where the status is 0 -- what the host build is held to against the
    oracle there, the device inherits."""
    cases = list(soak_family_case(oracle, fam))
    if fam != "degenerate":   # the translated case of tests/test_support_host.py: beta = b - a.xc cancels three digits
        cases += soak_family_case(oracle, fam, seed=sh.FAMILY_SEED[fam] + 100, shapes=((32, 4), (16, 3)), translate=1e3)
    if fam == "dup":
        for seed in (7, 8, 9, 10):
            cases += soak_family_case(oracle, "dup", seed=seed, shapes=sh.FOUND_SHAPES)
    for case in cases:
        for layout in ("shared", "own"):
            want_h, want_x, want_st = sh.run_case(L, case, layout)
            raw = batch.support_batch(case["A"], case["b"], case[layout][0], m=case["m"], xc=case["xc"], resolve=False)
            assert np.array_equal(raw["status"], want_st), (case["shape"], layout, np.argwhere(raw["status"] != want_st)[:5])
            ok = want_st == 0
            assert same_bits(raw["h"][ok], want_h[ok]) and same_bits(raw["x"][ok], want_x[ok]), (case["shape"], layout)
            assert np.all(np.isnan(raw["h"][want_st == 1])) and np.all(raw["h"][want_st == 3] == np.inf)


def test_found_fixtures_raw_equal_the_host_build(L):
    """tests/golden/found/support/*.npz: the three polytopes with the four status-0 answers that were not optimal, and the 54
    LPs on which the oracle is off -- statuses and bits of the host build (which tests/test_support_host.py holds against the
    oracle and the exact optimum by name)."""
    z = np.load(os.path.join(ROOT, "tests", "golden", "found", "support", "dup.npz"))
    calls = [(z["A_" + k[2:]][None], z["b_" + k[2:]][None], z["C_" + k[2:]], z["xc_" + k[2:]][None]) for k in z.files if k.startswith("A_")]
    calls += [(A[None], b[None], c[None], xc[None]) for _, A, b, c, xc, _, _ in sh.oracle_off_fixture()]
    assert len(calls) == 3 + 54
    for A, b, C_, xc in calls:
        want_h, want_x, want_st = sh.run(L, A, b, C_, xc)
        raw = batch.support_batch(A, b, C_, xc=xc, resolve=False)
        assert np.array_equal(raw["status"], want_st)
        ok = want_st == 0
        assert same_bits(raw["h"][ok], want_h[ok]) and same_bits(raw["x"][ok], want_x[ok])


@pytest.mark.parametrize("fam", ALL_FAMILIES)
def test_soak_families_resolved_equal_the_oracle(oracle, fam):
    """resolve=True on the same inputs: EVERY LP against the oracle with the extent rule, nothing left out -- the centre given
    (numpy in) and left to cheby_ball_batch (CUDA tensors in, and numpy for the shared layout).  A polytope the oracle finds
    empty gives 2 in every direction."""
    for case in soak_family_case(oracle, fam):
        A, b, m = case["A"], case["b"], case["m"]
        for layout in ("shared", "own"):
            C_, ost, oh, ox = case[layout]
            res = batch.support_batch(A, b, C_, m=m, xc=case["xc"])
            sh.check_against_oracle(A, b, m, C_, res["h"], res["x"], res["status"], ost, oh, ext=ox)
            At, bt, mt, Ct = dev(A, b, m, C_)
            rt = batch.support_batch(At, bt, Ct, m=mt)
            assert rt["h"].is_cuda
            sh.check_against_oracle(A, b, m, C_, rt["h"].cpu().numpy(), rt["x"].cpu().numpy(), rt["status"].cpu().numpy(), ost, oh, ext=ox)
            if layout == "shared":
                rn = batch.support_batch(A, b, C_, m=m)
                sh.check_against_oracle(A, b, m, C_, rn["h"], rn["x"], rn["status"], ost, oh, ext=ox)


@pytest.mark.parametrize("m_max,d", [(32, 4), (48, 4)])
def test_subset_batch_on_rows_a_hair_apart(oracle, m_max, d):
    """`dup`, B = 60: P against Q = the rows of P with every right-hand side moved to the oracle's h_P(a_i) + -1e-3 max(1, |h|)
    -- up on every row for the even polytopes (inside), down on some for the odd ones (not inside); a row in whose direction
    P is unbounded keeps its b (not inside).  No row is within 1e-4 of a tie; the verdicts are those of the oracle's h.  (An
    h that is too small -- a feasible vertex that is not the optimum -- turns "not inside" into "inside".)"""
    def make():
        rng = np.random.default_rng(700 + m_max)
        A, b, m = sh.family("dup", B=60, rng=rng, shape=(m_max, d))
        ost, oh = sh.oracle_support(oracle, A, b, m, A)
        return A, b, m, ost, oh, rng.random((60, m_max))
    A, b, m, ost, oh, u = sh.memo(("subset_dup", m_max), make)
    down = (u < 0.15) & (np.arange(60) % 2 == 1)[:, None]
    down[1::2, 0] = True
    assert np.all(np.isin(ost, (0, 3)))
    Qb = np.where(ost == 0, oh + np.where(down, -1e-3, 1e-3) * np.maximum(1.0, np.abs(oh)), b)
    gap = np.where(ost == 0, Qb - oh, -np.inf)
    assert np.all(np.abs(gap) > 1e-4)
    expect = (gap >= 0).all(axis=1)
    assert expect[1::2].sum() == 0 and expect[0::2].sum() >= 20
    got = batch.subset_batch(A, b, A, Qb, m=m, mq=m)
    assert got.dtype == bool and np.array_equal(got, expect), np.nonzero(got != expect)[0]
    gt = batch.subset_batch(*dev(A, b, A, Qb), m=dev(m)[0], mq=dev(m)[0])
    assert gt.is_cuda and np.array_equal(gt.cpu().numpy(), expect)


def test_soak_family_on_another_stream(oracle):
    """`dup` at (48, 4), K = 15, on a torch stream that is not the default one: the default stream's bits."""
    import torch
    case = soak_family_case(oracle, "dup")[5]
    C_ = case["shared"][0]
    full = batch.support_batch(case["A"], case["b"], C_, m=case["m"])
    At, bt, mt, Ct = dev(case["A"], case["b"], case["m"], C_)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        rs = batch.support_batch(At, bt, Ct, m=mt)
    side.synchronize()
    assert np.array_equal(rs["status"].cpu().numpy(), full["status"]) and same_bits(rs["h"].cpu().numpy(), full["h"])


@pytest.mark.parametrize("k", range(len(sh.SHAPES)))
def test_unbounded_family_resolved(oracle, k):
    """random_hpolytopes(bounded=False): 3 where the oracle says 3 (h = +inf), its optimum elsewhere; the centre comes
    from cheby_ball_batch, and polytopes whose ball is unbounded go through the fallback."""
    A, b, m = sh.family(k, bounded=False)
    C_ = sh.directions(k, A.shape[0], True)
    ost, oh = sh.oracle_support(oracle, A, b, m, C_)
    res = batch.support_batch(A, b, C_, m=m)
    sh.check_against_oracle(A, b, m, C_, res["h"], res["x"], res["status"], ost, oh)
    assert (ost == 3).sum() > 20 and np.all(res["h"][ost == 3] == np.inf)
    # with a centre given (the origin is strictly inside): the kernel settles these itself
    raw = batch.support_batch(A, b, C_, m=m, xc=np.zeros((A.shape[0], A.shape[2])), resolve=False)
    sh.check_against_oracle(A, b, m, C_, raw["h"], raw["x"], raw["status"], ost, oh, where=raw["status"] != 1)
    assert (raw["status"] == 1).sum() <= sh.HANDBACK_CAP * ost.size and (raw["status"] == 3).sum() > 20


def test_empty_flat_and_zero_direction(oracle):
    """An empty polytope: 2 in every direction.  A flat one (r = 0): no interior point, solved entirely by the fallback.
    A zero direction: h = 0, status 0 and a feasible x."""
    d = 3
    box = np.vstack([np.eye(d), -np.eye(d)])
    A = np.broadcast_to(box, (3, 6, d)).copy()
    b = np.array([[1.0, 1, 1, -2, 1, 1],      # x_0 <= 1 and x_0 >= 2: empty
                  [1.0, 1, 1, -1, 1, 1],      # x_0 = 1: flat
                  [1.0, 2, 3, 1, 2, 3]])
    C_ = np.vstack([np.eye(d), -np.eye(d), [[0.3, -0.2, 0.9]], np.zeros((1, d))])
    ost, oh = sh.oracle_support(oracle, A, b, None, C_)
    assert np.all(ost[0] == 2) and np.all(ost[1:] == 0)
    res = batch.support_batch(A, b, C_)
    sh.check_against_oracle(A, b, None, C_, res["h"], res["x"], res["status"], ost, oh)
    assert np.all(np.isnan(res["h"][0])) and np.all(res["h"][1:, 7] == 0.0)
    raw = batch.support_batch(A, b, C_, resolve=False)
    assert np.all(raw["status"][1] == 1) and np.all(raw["status"][2] == 0)
    assert np.all(np.isin(raw["status"][0], (1, 2)))
    At, bt, Ct = dev(A, b, C_)
    rt = batch.support_batch(At, bt, Ct)
    sh.check_against_oracle(A, b, None, C_, rt["h"].cpu().numpy(), rt["x"].cpu().numpy(), rt["status"].cpu().numpy(), ost, oh)


@pytest.mark.parametrize("m_max,d", [(16, 3), (32, 4)])
def test_axis_directions_equal_bbox_batch(m_max, d):
    """C = +-I: h is bbox_batch's ub / -lb within 1e-12 max(1, |h|) on every polytope bbox_batch settles, B = 300."""
    A, b, m = ragged(300, m_max, d, seed=77 + d)
    box = batch.bbox_batch(A, b, m)
    res = batch.support_batch(A, b, np.vstack([np.eye(d), -np.eye(d)]), m=m)
    ok = box["status"] == 0
    assert ok.sum() >= 295 and np.all(res["status"][ok] == 0)
    want = np.hstack([box["ub"], -box["lb"]])
    assert np.all(np.abs(res["h"][ok] - want[ok]) <= 1e-12 * np.maximum(1.0, np.abs(res["h"][ok])))


@pytest.mark.parametrize("m_max,d", [(20, 6), (70, 3)])
def test_shapes_without_a_shared_row_kernel(oracle, m_max, d):
    """d in 5..16 or more than 64 rows: the same interface through lpsolve_batch, K = 5, both layouts of C."""
    A, b = random_hpolytopes(12, m_max, d, seed=5 + d)
    rng = np.random.default_rng(d)
    for C_ in (rng.standard_normal((5, d)), rng.standard_normal((12, 5, d))):
        ost, oh = sh.oracle_support(oracle, A, b, None, C_)
        res = batch.support_batch(A, b, C_)
        sh.check_against_oracle(A, b, None, C_, res["h"], res["x"], res["status"], ost, oh)
        assert np.all(ost == 0)
    At, bt, Ct = dev(A, b, C_)
    rt = batch.support_batch(At, bt, Ct, points=False)
    assert rt["x"] is None
    sh.check_against_oracle(A, b, None, C_, rt["h"].cpu().numpy(), None, rt["status"].cpu().numpy(), ost, oh)


def test_without_points_and_on_another_stream():
    """points=False: no points, h bit for bit.  The _dev call on a torch stream that is not the default one: the same."""
    import torch
    A, b, m = ragged(70, 17, 3, seed=9)
    C_ = np.random.default_rng(9).standard_normal((70, 37, 3))
    full = batch.support_batch(A, b, C_, m=m)
    lean = batch.support_batch(A, b, C_, m=m, points=False)
    assert lean["x"] is None and np.array_equal(lean["status"], full["status"]) and same_bits(lean["h"], full["h"])
    At, bt, mt, Ct = dev(A, b, m, C_)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        rs = batch.support_batch(At, bt, Ct, m=mt)
        rl = batch.support_batch(At, bt, Ct, m=mt, points=False)
    side.synchronize()
    assert rl["x"] is None
    for r in (rs, rl):
        assert np.array_equal(r["status"].cpu().numpy(), full["status"]) and same_bits(r["h"].cpu().numpy(), full["h"])
    assert same_bits(rs["x"].cpu().numpy(), full["x"])


def test_subset_batch(oracle):
    """200 pairs: P against P scaled about its centre by 0.5 / 0.9 (not inside) and 1.1 / 2.0 (inside), and against a
    translated copy (not inside).  No pair is within 1e-3 of a tie; the verdicts are also those the oracle's h gives."""
    A, b, m = sh.family(2)
    B, m_max, d = A.shape
    xc = sh.centres(oracle, A, b, m)
    axc = np.einsum("pik,pk->pi", A, xc)
    t = np.random.default_rng(3).standard_normal((B, d))
    t *= 0.3 / np.linalg.norm(t, axis=1, keepdims=True)
    Qb = [axc + s * (b - axc) for s in (0.5, 0.9, 1.1, 2.0)] + [b + np.einsum("pik,pk->pi", A, t)]
    expect = np.repeat([False, False, True, True, False], B)
    PA, Pb, Pm = np.tile(A, (5, 1, 1)), np.tile(b, (5, 1)), np.tile(m, 5)
    Qb = np.vstack(Qb)
    assert PA.shape[0] == 200
    _, oh = sh.oracle_support(oracle, A, b, m, A)        # h_P(a_i) for every row of P, the rows of every Q
    gap = Qb - np.tile(oh, (5, 1))
    live = np.arange(m_max)[None, :] < Pm[:, None]
    gap = np.where(live, gap, np.inf)
    assert np.array_equal(gap.min(axis=1) >= 0, expect) and np.all(np.abs(gap.min(axis=1)) > 1e-3)
    got = batch.subset_batch(PA, Pb, PA, Qb, m=Pm, mq=Pm)
    assert got.dtype == bool and np.array_equal(got, expect)
    gt = batch.subset_batch(*dev(PA, Pb, PA, Qb), m=dev(Pm)[0], mq=dev(Pm)[0])
    assert gt.is_cuda and np.array_equal(gt.cpu().numpy(), expect)
    # an empty P is inside anything; an unbounded one is not inside a bounded Q
    E = np.array([[[1.0, 0.0], [-1.0, 0.0], [0.0, 1.0], [0.0, -1.0]]] * 2)
    Eb = np.array([[1.0, -2.0, 1.0, 1.0], [1.0, 1.0, 1.0, 1.0]])
    assert list(batch.subset_batch(E, Eb, E, np.ones((2, 4)) * 0.5, m=np.array([4, 3], np.int32))) == [True, False]


def test_c_abi_sizes():
    """plp_support_batch: d = 5 is a size error, B = 0 returns 0 without touching a pointer."""
    lib = _lib.load()
    ctx = _lib.context()
    z = np.zeros(64)
    st = np.zeros(8, np.int32)
    p = lambda a: C.c_void_p(a.ctypes.data)   # noqa: E731
    rc = lib.plp_support_batch(ctx.handle, 1, 4, 5, p(z), p(z), None, 2, p(z), 1, p(z), p(z), p(z), p(st))
    assert rc == _lib.PLP_EUNSUPPORTED and b"d=5" in lib.plp_last_error()
    assert lib.plp_support_batch(ctx.handle, 1, 65, 3, p(z), p(z), None, 2, p(z), 1, p(z), p(z), p(z), p(st)) == _lib.PLP_EUNSUPPORTED
    assert lib.plp_support_batch(ctx.handle, 1, 4, 3, p(z), p(z), None, 0, p(z), 1, p(z), p(z), p(z), p(st)) == _lib.PLP_EUNSUPPORTED
    assert lib.plp_support_batch(ctx.handle, 2 ** 30, 4, 3, p(z), p(z), None, 4, p(z), 1, p(z), p(z), p(z), p(st)) == _lib.PLP_EUNSUPPORTED
    assert lib.plp_support_batch(ctx.handle, 0, 4, 3, None, None, None, 2, None, 1, None, None, None, None) == 0
    assert lib.plp_support_batch_dev(ctx.handle, None, 0, 4, 3, None, None, None, 2, None, 1, None, None, None, None) == 0
    with pytest.raises(_lib.UnsupportedSize):
        batch._Backend(z).call("plp_support_batch", 1, 4, 5, z, z, None, 2, z, 1, z, z, z, st)
