"""GPU: pair_stacks / intersect_pairs / intersect_cross_sparse on CUDA tensors and the Polytope-level calls on 'hip'.

The stacks are held bit for bit against the host build of the same header and against numpy; the intersections integer for
integer (and the balls bit for bit at equal batch size) against reduce_batch + fm_emit on the stacks numpy builds; the
Polytope-level calls against the loop of Polytope.intersect and against the reference's results in
tests/golden/intersect_pairs.npz."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import intersect_pairs_cases as IC  # noqa: E402
import pair_stack_host as H  # noqa: E402
from host_build import same_bits  # noqa: E402

pytestmark = pytest.mark.gpu

# Chebyshev balls of the fused reduce across batch sizes (tile shapes), DESIGN 7: the same bits on data without ties in F1's
# ratio test, 4e-16 on unit-scale data where it ties (duplicated rows, cubes).  The bound here is that figure scaled to the
# data: 4e-16 * max(1, largest |coordinate| of the two balls compared) -- two ulp of a coordinate.  Where both sides run one
# batch of the same size the tests ask for the same bits instead.
BALL_ULPS = 4e-16


def _balls_apart(r1, x1, r2, x2):
    """Indices of the balls (r1[k], x1[k]) and (r2[k], x2[k]) that differ by more than the bound above."""
    r1, r2, x1, x2 = (np.asarray(v, dtype=float) for v in (r1, r2, x1, x2))
    scale = np.maximum(1.0, np.maximum(np.abs(x1).max(-1), np.abs(x2).max(-1)))
    scale = np.maximum(scale, np.maximum(np.abs(r1), np.abs(r2)))
    bad = (np.abs(r1 - r2) > BALL_ULPS * scale) | (np.abs(x1 - x2).max(-1) > BALL_ULPS * scale)
    return np.nonzero(bad)[0].tolist()


@pytest.fixture(scope="module")
def env():
    import torch
    import polytope_amd as pa
    assert torch.cuda.is_available()
    old = pa.solvers.default_solver
    pa.solvers.default_solver = "hip"
    yield torch, pa, torch.device("cuda:0")
    pa.solvers.default_solver = old


@pytest.fixture(scope="module")
def L(tmp_path_factory):
    return H.build(tmp_path_factory.mktemp("pair_stack_host"))


@pytest.fixture(scope="module")
def fixture():
    return IC.load_fixture()


def _dev(torch, dev, *arrays):
    return [None if a is None else torch.as_tensor(np.ascontiguousarray(a)).to(dev) for a in arrays]


def _host(res):
    return {k: (v.cpu().numpy() if hasattr(v, "cpu") else v) for k, v in res.items()}


# ------------------------------------------------------------------------------------------------ the stacks
@pytest.mark.parametrize("d", H.DIMS)
def test_pair_stacks_equal_host_build_and_numpy(env, L, d):
    torch, pa, dev = env
    for m_max in H.M_MAXES:
        A, b, m = H.table(d, m_max)          # (NaN at and beyond row m[p]: reading it would reach an output or a norm)
        pairs = H.all_pairs()
        got = _host(pa.pair_stacks(*_dev(torch, dev, A, b, pairs, m)))
        rc, hA, hb, hm = H.stacks(L, A, b, m, pairs)
        nA, nb, nm = H.numpy_stacks(A, b, m, pairs)
        assert rc == 0
        assert np.array_equal(got["m"], hm) and np.array_equal(got["m"], nm), (d, m_max)
        assert same_bits(got["A"], hA) and same_bits(got["b"], hb), (d, m_max)
        assert np.array_equal(got["A"], nA) and np.array_equal(got["b"], nb), (d, m_max)


def test_pair_stacks_k0_k1_and_without_m(env, L):
    torch, pa, dev = env
    A, b, m = H.table(3, 16, pad=0.0)
    At, bt, mt = _dev(torch, dev, A, b, m)
    got = pa.pair_stacks(At, bt, torch.zeros((0, 2), dtype=torch.int32, device=dev), mt)
    assert tuple(got["A"].shape) == (0, 32, 3) and tuple(got["b"].shape) == (0, 32) and tuple(got["m"].shape) == (0,)
    one = np.array([[4, 2]], np.int32)
    got = _host(pa.pair_stacks(At, bt, _dev(torch, dev, one)[0], mt))
    want = H.stacks(L, A, b, m, one)
    assert same_bits(got["A"], want[1]) and same_bits(got["b"], want[2]) and np.array_equal(got["m"], want[3])
    rng = np.random.default_rng(3)
    A2, b2 = rng.standard_normal((7, 16, 3)) * 2.0, rng.standard_normal((7, 16))
    got = _host(pa.pair_stacks(*_dev(torch, dev, A2, b2, H.all_pairs())))
    want = H.stacks(L, A2, b2, None, H.all_pairs())
    assert same_bits(got["A"], want[1]) and same_bits(got["b"], want[2]) and np.all(got["m"] == 32)
    # the host-pointer form: the same stacks, and a bad pair is rejected before anything runs
    got = pa.pair_stacks(A, b, one, m)
    want = H.stacks(L, A, b, m, one)
    assert same_bits(got["A"], want[1]) and same_bits(got["b"], want[2]) and np.array_equal(got["m"], want[3])
    with pytest.raises(ValueError, match="two different cells"):
        pa.pair_stacks(A, b, np.array([[0, 1], [3, 3]], np.int32), m)
    with pytest.raises(ValueError, match="two different cells"):
        pa.batch.intersect_pairs(A, b, np.array([[0, 7]], np.int32), m)


# ------------------------------------------------------------------------------------------------ intersect_pairs (packed)
def _cells(d, m_max, n=12, seed=0):
    """n cells of ragged row counts around centres a fraction of their size apart (they overlap, touch or lie apart): box
    rows first where 2 d of them fit, random unit cuts beyond -> A[n, m_max, d], b, m."""
    rng = np.random.default_rng(97 * d + m_max + 1009 * seed)
    A, b = np.zeros((n, m_max, d)), np.zeros((n, m_max))
    m = rng.integers(max(1, m_max // 2), m_max + 1, n).astype(np.int32)
    for p in range(n):
        c = rng.uniform(-1.0, 1.0, d)
        rows = rng.standard_normal((m[p], d))
        rows /= np.linalg.norm(rows, axis=1, keepdims=True)
        if m[p] >= 2 * d:
            rows[:2 * d] = np.vstack([np.eye(d), -np.eye(d)])
        A[p, :m[p]] = rows
        b[p, :m[p]] = rows @ c + rng.uniform(0.5, 1.5, m[p])
    return A, b, m


def _ordered_pairs(n):
    return np.array([(i, j) for i in range(n) for j in range(n) if i != j], dtype=np.int32)


@pytest.mark.parametrize("m_max", [8, 16, 32])
@pytest.mark.parametrize("d", [2, 3, 4, 6, 8, 9, 12, 16])
def test_intersect_pairs_equals_reduce_batch_on_numpy_stacks(env, d, m_max):
    torch, pa, dev = env
    A, b, m = _cells(d, m_max)
    pairs = _ordered_pairs(12)
    At, bt, mt, pt = _dev(torch, dev, A, b, m, pairs)
    sA, sb, sm = H.numpy_stacks(A, b, m, pairs)
    sAt, sbt, smt = _dev(torch, dev, sA, sb, sm)
    want = _host(pa.reduce_batch(sAt, sbt, m=smt))
    got = _host(pa.batch.intersect_pairs(At, bt, pt, m=mt))
    assert np.array_equal(got["ms"], sm)
    for k in ("keep", "flags", "nlp"):
        assert np.array_equal(got[k].astype(np.int64), want[k].astype(np.int64)), k
    # one batch of the same size on both sides: the balls are the same bits
    assert same_bits(got["r"], want["r"]) and same_bits(got["xc"], want["xc"])
    # the rows: fm_emit(col = -1) of the numpy stacks under reduce_batch's keep and flags, bit for bit
    mo_max = int(got["A"].shape[1])
    rows = np.array([bin(int(k) & (2 ** 64 - 1)).count("1") for k in want["keep"]])
    rows[(want["flags"] & (1 | 8 | 32)) != 0] = 0
    assert mo_max == max(1, int(rows.max()))
    eA, eb, em = pa.batch.fm_emit(sAt, sbt, -1, mo_max, m=smt, keep=_dev(torch, dev, want["keep"].view(np.int64))[0],
                                  flags=_dev(torch, dev, want["flags"])[0])
    assert np.array_equal(got["m"], em.cpu().numpy()) and np.array_equal(got["m"], rows)
    assert same_bits(got["A"], eA.cpu().numpy()) and same_bits(got["b"], eb.cpu().numpy())
    # three chunks with a ragged tail: verdict-level outputs and rows never differ, the balls within the documented bound
    ch = _host(pa.batch.intersect_pairs(At, bt, pt, m=mt, chunk=50))
    for k in ("keep", "flags", "nlp", "ms", "m"):
        assert np.array_equal(ch[k], got[k]), k
    assert same_bits(ch["A"], got["A"]) and same_bits(ch["b"], got["b"])
    ball = (got["flags"] & 1) == 0
    dr = np.abs(ch["r"][ball] - got["r"][ball])
    dx = np.abs(ch["xc"][ball] - got["xc"][ball])
    print("d=%d m_max=%d: %d balls, max |dr| %.3g, max |dxc| %.3g across chunkings" % (
        d, m_max, int(ball.sum()), dr.max() if dr.size else 0.0, dx.max() if dx.size else 0.0))
    # the balls that differ across chunkings by more than the bound, by index: none expected
    assert _balls_apart(ch["r"][ball], ch["xc"][ball], got["r"][ball], got["xc"][ball]) == []
    # mo_max passed too small: -1 for the results that do not fit, the others as before; and the one-pass form agrees
    if mo_max > 1:
        small = _host(pa.batch.intersect_pairs(At, bt, pt, m=mt, mo_max=mo_max - 1))
        over = rows > mo_max - 1
        assert over.any() and np.all(small["m"][over] == -1) and np.array_equal(small["m"][~over], rows[~over])
        assert same_bits(small["A"][~over], got["A"][~over][:, :mo_max - 1]) and np.array_equal(small["keep"], got["keep"])
    exact = _host(pa.batch.intersect_pairs(At, bt, pt, m=mt, mo_max=mo_max))
    assert np.array_equal(exact["m"], got["m"]) and same_bits(exact["A"], got["A"]) and same_bits(exact["b"], got["b"])


def test_bad_pairs_are_flagged_and_leave_the_rest_alone(env):
    torch, pa, dev = env
    A, b, m = _cells(3, 8)
    good = _ordered_pairs(12)[:40]
    bad = np.array(H.BAD_PAIRS[:2] + ((12, 0), (0, 12), (3, 3)) + H.BAD_PAIRS[5:], dtype=np.int64).astype(np.int32)
    at = [0, 7, 8, 20, 33, 45, 46]          # (positions of the bad pairs in the list, the last two at its end)
    listed = np.insert(good, [0, 6, 6, 17, 29, 40, 40], bad, axis=0)
    assert np.array_equal(listed[at], bad)
    At, bt, mt, pt, gt = _dev(torch, dev, A, b, m, listed, good)
    got = _host(pa.batch.intersect_pairs(At, bt, pt, m=mt))
    want = _host(pa.batch.intersect_pairs(At, bt, gt, m=mt, mo_max=int(got["A"].shape[1])))
    rest = np.setdiff1d(np.arange(len(listed)), at)
    assert np.all(got["flags"][at] == (pa.batch.RF_EMPTY | pa.batch.RF_BADPAIR))
    assert np.all((got["flags"][rest] & pa.batch.RF_BADPAIR) == 0)
    for k in ("keep", "r", "nlp", "ms", "m"):
        assert np.all(got[k][at] == 0), k
    assert np.all(np.isnan(got["xc"][at])) and np.all(got["A"][at] == 0.0) and np.all(got["b"][at] == 0.0)
    for k in ("keep", "flags", "nlp", "ms", "m"):
        assert np.array_equal(got[k][rest], want[k]), k
    assert same_bits(got["A"][rest], want["A"]) and same_bits(got["b"][rest], want["b"])
    st = _host(pa.pair_stacks(At, bt, pt, mt))
    assert np.all(st["m"][at] == 0) and np.all(st["A"][at] == 0.0) and np.all(st["b"][at] == 0.0)


def test_host_pointer_form_equals_the_device_form(env):
    torch, pa, dev = env
    A, b, m = _cells(3, 8)
    pairs = _ordered_pairs(12)[:30]
    host = pa.batch.intersect_pairs(A, b, pairs, m=m, chunk=7)          # numpy in: numpy out, through the HostCall
    assert all(isinstance(v, np.ndarray) for v in host.values())
    At, bt, mt, pt = _dev(torch, dev, A, b, m, pairs)
    want = _host(pa.batch.intersect_pairs(At, bt, pt, m=mt, chunk=7))
    for k in ("keep", "flags", "nlp", "ms", "m"):
        assert np.array_equal(host[k].astype(np.int64), want[k].astype(np.int64)), k
    for k in ("r", "xc", "A", "b"):
        assert same_bits(host[k], want[k]), k
    one = pa.batch.intersect_pairs(A, b, pairs, m=m, chunk=7, mo_max=int(want["A"].shape[1]))
    assert np.array_equal(one["m"], want["m"]) and same_bits(one["A"], want["A"]) and same_bits(one["b"], want["b"])


def test_empty_list_with_sizes_outside_the_envelope_and_no_row_slots(env):
    """The C calls report 2 m_max > 64 or d > 16 also for an empty list; mo_max = 0 still emits: m = -1 where rows exist."""
    import ctypes as C
    torch, pa, dev = env
    from polytope_amd import _lib
    lib, ctx = _lib.load(), _lib.context(0)
    for m_max, d in ((33, 2), (4, 17)):
        assert lib.plp_pair_stacks(ctx.handle, 3, m_max, d, None, None, None, 0, None, None, None, None) == _lib.PLP_EUNSUPPORTED
        assert lib.plp_pair_stacks_dev(ctx.handle, None, 3, m_max, d, None, None, None, 0, None, None, None, None) \
            == _lib.PLP_EUNSUPPORTED
        assert lib.plp_intersect_pairs_dev(ctx.handle, None, 3, m_max, d, None, None, None, 1e-7, 0, None, 0, None, None, None,
                                           None, None, None, 0, None, None, None) == _lib.PLP_EUNSUPPORTED
    assert lib.plp_pair_stacks(ctx.handle, 3, 32, 16, None, None, None, 0, None, None, None, None) == _lib.PLP_OK
    assert lib.plp_pair_chunk_default(8, 4) == (32 << 20) // (16 * 5 * 8) and lib.plp_pair_chunk_default(32, 16) == 3855
    A, b, m = _cells(3, 8)
    pairs = _ordered_pairs(12)[:30]
    At, bt, mt, pt = _dev(torch, dev, A, b, m, pairs)
    want = _host(pa.batch.intersect_pairs(At, bt, pt, m=mt))
    assert (want["m"] > 0).any() and (want["m"] == 0).any()
    for args in ((At, bt, pt, mt), (A, b, pairs, m)):
        got = _host(pa.batch.intersect_pairs(args[0], args[1], args[2], m=args[3], mo_max=0))
        assert tuple(got["A"].shape) == (30, 0, 3) and tuple(got["b"].shape) == (30, 0)
        assert np.array_equal(got["m"], np.where(want["m"] > 0, -1, 0))
        assert np.array_equal(got["keep"].astype(np.int64), want["keep"].astype(np.int64))


def test_empty_list(env):
    torch, pa, dev = env
    A, b, m = _cells(3, 8)
    At, bt, mt = _dev(torch, dev, A, b, m)
    got = pa.batch.intersect_pairs(At, bt, torch.zeros((0, 2), dtype=torch.int32, device=dev), m=mt)
    assert tuple(got["keep"].shape) == (0,) and tuple(got["xc"].shape) == (0, 3) and tuple(got["A"].shape) == (0, 1, 3)


# ------------------------------------------------------------------------------------------------ Polytope level on 'hip'
def _ball_close(p, q):
    """The cached balls of two results: both absent, or equal within the bound above (the batch call and the single call
    run batches of different sizes)."""
    if p._chebXc is None or q._chebXc is None:
        return p._chebXc is None and q._chebXc is None
    return _balls_apart([float(p._chebR)], [np.asarray(p._chebXc).ravel()], [float(q._chebR)],
                        [np.asarray(q._chebXc).ravel()]) == []


@pytest.mark.parametrize("fam", IC.FAMILIES)
def test_polytope_level_equals_the_loop_and_the_fixture(env, fixture, fam):
    torch, pa, dev = env
    f = fixture[fam]
    cells = IC.cells_of(pa, f)
    got = pa.intersect_pairs(cells, f["pairs"])
    loop_cells = IC.cells_of(pa, f)
    want = [loop_cells[i].intersect(loop_cells[j]) for i, j in f["pairs"]]
    assert len(got) == len(want) == len(f["pairs"])      # no pair is skipped
    off_fixture, off_ball = [], []
    for t, (g, w) in enumerate(zip(got, want)):
        assert g.A.shape == w.A.shape and np.array_equal(g.A, w.A) and np.array_equal(g.b, w.b), t
        assert g.minrep == w.minrep, t
        if not _ball_close(g, w):
            off_ball.append(t)
            print("pair %d: r %r / %r, xc %r / %r" % (t, g._chebR, w._chebR, g._chebXc, w._chebXc))
        how = IC.differs_from_fixture(f, t, g)
        if how is not None:
            # allowed only where the existing single call on 'hip' differs from the reference too
            assert IC.differs_from_fixture(f, t, w) is not None, (t, how)
            off_fixture.append(t)
    assert off_fixture == []      # the pairs that differ from the reference, by index: none expected
    assert off_ball == []         # the pairs whose cached ball differs from the single call's beyond the bound: none expected


def test_polytope_level_mixed_operands(env):
    torch, pa, dev = env
    a, b = pa.box2poly([[0, 1], [0, 1]]), pa.box2poly([[0.5, 2], [0.5, 2]])
    flat = pa.Polytope(np.array([[1.0, 0], [-1.0, 0], [0, 1.0], [0, -1.0]]), np.array([1.0, -1.0, 1.0, 0.0]))
    rng = np.random.default_rng(1)
    rows = rng.standard_normal((40, 2))
    big = pa.Polytope(rows, np.abs(rows).sum(1) * 0.0 + 3.0)      # 40 rows: outside the envelope, the single call
    cells = [a, b, flat, pa.Polytope(), big]
    pairs = [(0, 1), (0, 2), (3, 0), (0, 0), (1, 0), (4, 0), (1, 4)]
    got = pa.intersect_pairs(cells, pairs)
    want = [cells[i].intersect(cells[j]) for i, j in pairs]
    for t, (g, w) in enumerate(zip(got, want)):
        assert g.A.shape == w.A.shape and np.array_equal(g.A, w.A) and np.array_equal(g.b, w.b) and g.minrep == w.minrep, t
    with pytest.raises(Exception, match="different dimension"):
        pa.intersect_pairs([a, pa.box2poly([[0, 1]] * 3)], [(0, 1)])


# ------------------------------------------------------------------------------------------------ the sparse cross form
def _family_table(f):
    return f["A"], f["b"], f["m"]


@pytest.mark.parametrize("fam,n1", [("a", 18), ("b3", 2)])
def test_intersect_cross_sparse_equals_all_pairs(env, fixture, fam, n1):
    torch, pa, dev = env
    # (the cells as Polytopes hold them: normalised rows, as _table_of packs them)
    cells = IC.cells_of(pa, fixture[fam])
    A, b, m = pa.polytope._pack(cells)
    n = len(cells)
    At, bt, mt = _dev(torch, dev, A, b, m)
    every = np.array([(i, j) for i in range(n1) for j in range(n1, n)], dtype=np.int32)
    dense = _host(pa.batch.intersect_pairs(At, bt, _dev(torch, dev, every)[0], m=mt))
    live = (dense["flags"] & 1) == 0
    want_pairs = every[live] - np.array([0, n1], np.int32)
    lb, ub = pa.bbox_batch(At, bt, mt)["lb"], pa.bbox_batch(At, bt, mt)["ub"]
    for kw in ({}, {"max_candidates": 7}, {"boxes": (lb, ub)}):
        got = _host(pa.intersect_cross_sparse(At, bt, n1, m=mt, **kw))
        assert got["pairs"].dtype == np.int32 and np.array_equal(got["pairs"], want_pairs), kw
        assert got["open"].size == 0 and got["ncand"] <= len(every)
        mo = int(got["A"].shape[1])
        assert np.array_equal(got["m"], dense["m"][live])
        assert same_bits(got["A"], dense["A"][live][:, :mo]) and same_bits(got["b"], dense["b"][live][:, :mo])
        assert _balls_apart(got["r"], got["xc"], dense["r"][live], dense["xc"][live]) == [], kw
    # the pairs are the nonzeros of overlap_cross, except those listed here by index with the reason (the reduce's F1
    # against the pair engine's careful pass): none expected
    ov = torch.nonzero(pa.batch.overlap_cross(At, bt, n1, m=mt)).to(torch.int32).cpu().numpy()
    differing = sorted({tuple(p) for p in want_pairs.tolist()} ^ {tuple(p) for p in ov.tolist()})
    assert differing == []
    if fam == "a":
        assert len(want_pairs) == 75 and got["ncand"] < len(every)     # the cull culls


def test_overlay_on_hip_equals_the_fixture(env, fixture):
    torch, pa, dev = env
    f = fixture["a"]
    cells = IC.cells_of(pa, f)
    got, parents = pa.overlay(cells[:18], cells[18:])
    live = np.nonzero(f["rm"] > 0)[0]
    want = np.stack([f["pairs"][live, 0], f["pairs"][live, 1] - 18], 1).astype(np.int32)
    assert np.array_equal(parents, want) and len(got) == 75
    single = [cells[i].intersect(cells[18 + j]) for i, j in parents]
    for q, w, t in zip(got, single, live):
        assert IC.differs_from_fixture(f, int(t), q) is None, (t, IC.differs_from_fixture(f, int(t), q))
        assert np.array_equal(q.A, w.A) and np.array_equal(q.b, w.b) and q.minrep == w.minrep and _ball_close(q, w)
    from polytope_amd._lib import UnsupportedSize
    with pytest.raises(UnsupportedSize):
        pa.overlay([cells[0]], [pa.Region([cells[1], cells[2]])])
