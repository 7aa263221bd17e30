"""GPU: hull_enum_kernel (csrc/plp_hull_enum.hip) through batch.hull_batch and the C ABI, against the host build of the same
source (tests/cabi/hull_enum_host.cpp: status, count, on and basis identical, A and b bit for bit), against the reference's
quickhull() (tests/golden/g30_hull.npz; the comparison and the cap on unpinned cases are those of tests/test_hull_host.py,
tests/hull_host.py: compare / check_cases) and, as a round trip, against extreme_batch and reduce_batch."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from polytope_amd import _lib, batch  # noqa: E402
from polytope_amd.synth import random_hpolytopes  # noqa: E402
import extreme_host as xh  # noqa: E402
import hull_host as hh  # noqa: E402
import cap_sweep  # noqa: E402
from cap_sweep import subset_rank  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def L(tmp_path_factory):
    return hh.build(tmp_path_factory.mktemp("hull_host"))


def dev(*arrays):
    import torch
    return [None if a is None else torch.as_tensor(a).to("cuda:0") for a in arrays]


def host(res):
    """A result of CUDA tensors as numpy arrays (`on` back as uint64)."""
    out = {k: None if v is None else v.cpu().numpy() for k, v in res.items()}
    out["on"] = out["on"].view(np.uint64)
    return out


def raw(X, n, keep, f_max, basis=True):
    """The kernel with an explicit keep mask (the public call takes none: one level below it)."""
    be = batch._Backend(X)
    B, n_max, d = X.shape
    res = dict(A=be.out((B, f_max, d)), b=be.out((B, f_max)), on=be.out((B, f_max), np.uint64), count=be.out((B,), np.int32),
               status=be.out((B,), np.int32), basis=be.out((B, f_max, d), np.int32) if basis else None)
    be.call("plp_hull_batch", B, n_max, d, X, n, keep, f_max, res["A"], res["b"], res["on"], res["count"], res["basis"],
            res["status"])
    return res


# ------------------------------------------------------------------------------------------ the host build, bit for bit
@pytest.mark.parametrize("n_max,d", [(2, 1), (5, 2), (17, 2), (64, 2), (16, 3), (33, 3), (64, 3), (12, 4), (32, 4), (64, 4)])
def test_kernel_equals_the_host_build(L, n_max, d):
    """An explicit keep mask against the host build: identical status, count, on and basis, A and b bit for bit.
    B in {1, 5, 257}; (64, 4), 635 376 candidates per set, at B = 5.  One round and many, candidate counts that are no
    multiple of 64, ragged n, keep masks with holes, exact repeats, lattice sets, one flat set per batch (tests/hull_host.py:
    raw_batch).  CUDA tensors give the same bits."""
    for B in ((5,) if (n_max, d) == (64, 4) else (1, 5, 257)):
        X, n, keep = hh.raw_batch(B, n_max, d, seed=89 * d + n_max + B)
        f_max = hh.fmax_for(d, n_max)
        want = hh.run(L, X, n, keep, f_max)
        got = raw(X, n, keep, f_max)
        assert hh.same_result(got, want) is None, (B, hh.same_result(got, want))
        assert (want["status"] == hh.HS_OK).any() and (B == 1 or want["status"][B // 2] == hh.HS_FLAT)
        if B != 5:
            Xt, nt, kt = dev(X, n, keep.view(np.int64))
            gt = raw(Xt, nt, kt, f_max, basis=(B == 1))
            assert gt["A"].is_cuda and hh.same_result(host(gt), want, basis=(B == 1)) is None
        # the public call: every point live
        res = batch.hull_batch(X, n=n, f_max=f_max, basis=True)
        assert hh.same_result(res, hh.run(L, X, n, None, f_max)) is None
    if n_max >= 32 and d >= 3:   # in some set the second facet was accepted in a later round of 64 than the first
        later = 0
        for q in range(B):
            if want["count"][q] >= 2:
                live = sorted(i for i in hh.bits(keep[q]) if i < n[q])
                r0, r1 = (subset_rank([live.index(int(i)) for i in want["basis"][q, f]], len(live)) for f in (0, 1))
                later += r0 // 64 != r1 // 64
        assert later > 0


def test_cap_sweep_equals_the_host_build(L):
    """Overflow reached in a LATER round of 64 (tests/cap_sweep.py; the host build's own sweep is in test_hull_host.py): at
    every cap from 1 to the full count + 1 the kernel's list is the host build's bit for bit, for the set twice in one
    launch."""
    for X in cap_sweep.hull_members():
        X2 = np.stack([X, X])
        full = int(hh.run(L, X[None])["count"][0])
        for k in range(1, full + 2):
            want = hh.run(L, X2, f_max=k)
            assert hh.same_result(raw(X2, None, None, k), want) is None, k
            assert (want["status"] == (hh.HS_OVERFLOW if k < full else hh.HS_OK)).all() and (want["count"] == min(k, full)).all()


def test_overflow_on_the_cube():
    import itertools
    cube = np.array(list(itertools.product([-1.0, 1.0], repeat=3)))[None]
    full = batch.hull_batch(cube, basis=True)
    assert full["status"][0] == batch.HS_OK and full["count"][0] == 6 and full["A"].shape == (1, 12, 3)
    cut = batch.hull_batch(cube, f_max=3, basis=True)
    assert cut["status"][0] == batch.HS_OVERFLOW and cut["count"][0] == 3
    assert hh.same_bits(cut["A"], full["A"][:, :3]) and hh.same_bits(cut["b"], full["b"][:, :3])
    assert np.array_equal(cut["on"], full["on"][:, :3]) and np.array_equal(cut["basis"], full["basis"][:, :3])
    assert batch.hull_batch(cube, f_max=6)["status"][0] == batch.HS_OK
    rows = {tuple(np.r_[a, beta] + 0.0) for a, beta in zip(full["A"][0, :6], full["b"][0, :6])}
    assert rows == {tuple(np.r_[s * np.eye(3)[k], 1.0] + 0.0) for k in range(3) for s in (1.0, -1.0)}
    assert all(len(hh.bits(w)) == 4 for w in full["on"][0, :6]) and np.all(full["on"][0, 6:] == 0)


# ------------------------------------------------------------------------------------------ the fixture
@pytest.fixture(scope="module")
def fixture_runs():
    """The whole fixture through hull_batch, one call per dimension, with numpy arrays and with CUDA tensors -> (cases,
    numpy results, tensor results as numpy); a result is (A, b, count, status, on) per case."""
    cases = hh.fixture()
    out_np, out_t = [None] * len(cases), [None] * len(cases)
    for d in (2, 3, 4):
        sel, X, n = hh.pack(cases, d)
        rn = batch.hull_batch(X, n=n)
        Xt, nt = dev(X, n)
        rt = batch.hull_batch(Xt, n=nt)
        assert rt["A"].is_cuda and rt["basis"] is None and rt["A"].shape == rn["A"].shape
        rt = host(rt)
        for k, i in enumerate(sel):
            out_np[i] = (rn["A"][k], rn["b"][k], rn["count"][k], rn["status"][k], rn["on"][k])
            out_t[i] = (rt["A"][k], rt["b"][k], rt["count"][k], rt["status"][k], rt["on"][k])
    return cases, out_np, out_t


def test_fixture_numpy_input(fixture_runs):
    cases, out_np, _ = fixture_runs
    assert hh.check_cases(cases, [r[:4] for r in out_np], "hull_batch, numpy") <= 1
    seen = {int(r[3]) for r in out_np}
    assert seen == {batch.HS_OK, batch.HS_FLAT}
    for A, b, count, status, on in out_np:
        assert (status == batch.HS_FLAT) == (count == 0)
        assert np.all(np.isfinite(A[:count])) and np.all(np.isnan(A[count:])) and np.all(np.isnan(b[count:])) and np.all(on[count:] == 0)


def test_fixture_cuda_tensors_same_bits(fixture_runs):
    cases, out_np, out_t = fixture_runs
    hh.check_cases(cases, [r[:4] for r in out_t], "hull_batch, CUDA tensors")
    for (An, bn, cn, sn, on), (At, bt, ct, st, ot) in zip(out_np, out_t):
        assert cn == ct and sn == st and hh.same_bits(An, At) and hh.same_bits(bn, bt) and np.array_equal(on, ot)


# ------------------------------------------------------------------------------------------ the round trip
@pytest.mark.parametrize("m,d", [(16, 3), (12, 2), (12, 4)])
def test_round_trip_rows_to_vertices_to_rows(m, d):
    """hull_batch(extreme_batch(P)["V"], n=count) returns the kept rows of reduce_batch(P), normalised, as a set: equal
    counts and every kept row within MATCH (1e-8, tests/extreme_host.py) of one of ours in |dA|_inf + |db| / E, E =
    max(1, |V|_inf) the extent.  CUDA tensors: V carries NaN beyond count, which the host-pointer entry refuses."""
    A, b = random_hpolytopes(64, m, d, seed=40 + d, bounded=True)
    At, bt = dev(A, b)
    ex = batch.extreme_batch(At, bt)
    assert bool((ex["status"] == batch.XS_OK).all())
    hb = host(batch.hull_batch(ex["V"], n=ex["count"]))
    V, vc = ex["V"].cpu().numpy(), ex["count"].cpu().numpy()
    keep = batch.keep_to_bool(batch.reduce_batch(A, b)["keep"], m)
    assert np.all(hb["status"] == batch.HS_OK)
    for p in range(64):
        nrm = np.linalg.norm(A[p, keep[p]], axis=1)
        RA, Rb = A[p, keep[p]] / nrm[:, None], b[p, keep[p]] / nrm
        cnt = int(hb["count"][p])
        assert cnt == len(Rb), (p, cnt, len(Rb))
        E = max(1.0, float(np.abs(V[p, :vc[p]]).max()))
        for a, beta in zip(RA, Rb):
            dist = np.min(np.max(np.abs(hb["A"][p, :cnt] - a), axis=1) + np.abs(hb["b"][p, :cnt] - beta) / E)
            assert dist <= xh.MATCH, (p, dist)
        # every vertex lies on at least d facets
        used = np.zeros(64, int)
        for w in hb["on"][p, :cnt]:
            for i in hh.bits(w):
                used[i] += 1
        assert np.all(used[:vc[p]] >= d) and np.all(used[vc[p]:] == 0)


@pytest.mark.parametrize("n,d", [(16, 3), (12, 2), (12, 4)])
def test_round_trip_points_to_rows_to_vertices(n, d):
    """extreme_batch(hull_batch(X)) returns exactly the points flagged in some `on` word -- for points in general position
    those are the vertices -- to MATCH of the extent.  reduce=False: the rows of a hull of points in general position are
    irredundant and bounded as they come, and reduce() is not exact on them -- with reduce=True set 37 of the (12, 4)
    batch loses two true facets (each 1.6e-5 from being implied by the other 27 rows; the oracle's reduce() drops the same
    two) and 13 vertices come back where the set has 11."""
    X = np.random.default_rng(50 + d).standard_normal((64, n, d))
    hb = batch.hull_batch(dev(X)[0])
    assert bool((hb["status"] == batch.HS_OK).all())
    ex = batch.extreme_batch(hb["A"], hb["b"], m=hb["count"], reduce=False)
    V, vc, st = ex["V"].cpu().numpy(), ex["count"].cpu().numpy(), ex["status"].cpu().numpy()
    on, fc = hb["on"].cpu().numpy().view(np.uint64), hb["count"].cpu().numpy()
    assert np.all(st == batch.XS_OK)
    for p in range(64):
        flagged = sorted(set().union(*[hh.bits(w) for w in on[p, :fc[p]]]))
        assert len(flagged) == vc[p], (p, flagged, vc[p])
        E = max(1.0, float(np.abs(X[p]).max()))
        near = np.abs(V[p, :vc[p], None, :] - X[p][None, flagged, :]).max(axis=2) <= xh.MATCH * E
        assert near.any(axis=0).all() and near.any(axis=1).all()


# ------------------------------------------------------------------------------------------ the C ABI
def test_c_abi_host_pointer_entry(L):
    lib = _lib.load()
    ctx = _lib.context()
    p = lambda a: None if a is None else C.c_void_p(a.ctypes.data)   # noqa: E731
    X, n, keep = hh.raw_batch(37, 16, 3, seed=5)
    f_max = hh.fmax_for(3, 16)
    want = hh.run(L, X, n, keep, f_max)
    got = dict(A=np.empty((37, f_max, 3)), b=np.empty((37, f_max)), on=np.empty((37, f_max), np.uint64),
               basis=np.empty((37, f_max, 3), np.int32), count=np.empty(37, np.int32), status=np.empty(37, np.int32))
    rc = lib.plp_hull_batch(ctx.handle, 37, 16, 3, p(X), p(n), p(keep), f_max, p(got["A"]), p(got["b"]), p(got["on"]),
                            p(got["count"]), p(got["basis"]), p(got["status"]))
    assert rc == 0 and hh.same_result(got, want) is None
    # without n, keep and basis: every point of every set
    rc = lib.plp_hull_batch(ctx.handle, 37, 16, 3, p(X), None, None, f_max, p(got["A"]), p(got["b"]), p(got["on"]),
                            p(got["count"]), None, p(got["status"]))
    assert rc == 0 and hh.same_result(got, hh.run(L, X, None, None, f_max), basis=False) is None
    # the envelope
    z, i4, u8 = np.zeros(512), np.zeros(8, np.int32), np.zeros(8, np.uint64)
    call = lambda B, n_max, d, f: lib.plp_hull_batch(ctx.handle, B, n_max, d, p(z), None, None, f, p(z), p(z), p(u8), p(i4), None, p(i4))   # noqa: E731
    assert call(1, 4, 5, 4) == _lib.PLP_EUNSUPPORTED and b"d=5" in lib.plp_last_error()
    assert call(1, 4, 0, 4) == _lib.PLP_EUNSUPPORTED and b"d=0" in lib.plp_last_error()
    assert call(1, 65, 3, 4) == _lib.PLP_EUNSUPPORTED and b"n_max=65" in lib.plp_last_error()
    assert call(2 ** 31, 4, 3, 4) == _lib.PLP_EUNSUPPORTED and b"B=2147483648" in lib.plp_last_error()
    assert call(1, 4, 3, 0) == _lib.PLP_EINVAL and b"f_max=0" in lib.plp_last_error()
    assert lib.plp_hull_batch(ctx.handle, 0, 4, 3, None, None, None, 4, None, None, None, None, None, None) == 0
    assert lib.plp_hull_batch_dev(ctx.handle, None, 0, 4, 3, None, None, None, 4, None, None, None, None, None, None) == 0
    empty = batch.hull_batch(np.zeros((0, 6, 3)))
    assert empty["A"].shape == (0, 8, 3) and empty["count"].shape == (0,) and empty["basis"] is None
