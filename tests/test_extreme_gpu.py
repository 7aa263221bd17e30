"""GPU: extreme_kernel (csrc/plp_extreme.hip) through batch.extreme_batch and the C ABI, against the host build of the same
source (tests/cabi/extreme_host.cpp: status, count and basis identical, V bit for bit) and, through the public call with
reduce=True, against the reference's extreme() (tests/golden/g29_extreme.npz; the comparison and the cap on unpinned cases
are those of tests/test_extreme_host.py, tests/extreme_host.py: compare / check_cases)."""
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
import cap_sweep  # noqa: E402
from host_build import same_bits  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def L(tmp_path_factory):
    return xh.build(tmp_path_factory.mktemp("extreme_host"))


def dev(*arrays):
    import torch
    return [None if a is None else torch.as_tensor(a).to("cuda:0") for a in arrays]


def raw_batch(B, m_max, d, seed):
    """Ragged random polytopes with zeroed padding rows, an exact copy of a row in every second one (a vertex with several
    bases: the filter has something to drop, within a round and across rounds), a zero row in every fifth, and a keep mask
    with holes."""
    rng = np.random.default_rng(seed)
    A, b = random_hpolytopes(B, m_max, d, seed=seed)
    m = rng.integers(min(m_max, d + 1), m_max + 1, size=B).astype(np.int32)
    m[0] = m_max
    for p in range(B):
        if p % 2 and m[p] > 3:
            A[p, 3], b[p, 3] = A[p, 0], b[p, 0]
        if p % 5 == 4:
            A[p, m[p] - 1], b[p, m[p] - 1] = 0.0, 0.5
        A[p, m[p]:] = 0.0
        b[p, m[p]:] = 0.0
    keep = np.zeros(B, np.uint64)
    for p in range(B):
        mask = rng.random(64) < 0.85
        mask[:min(2 * d, 64)] = True
        keep[p] = xh.keep_word(mask)
    keep[0] = np.uint64(2 ** 64 - 1)
    return A, b, m, keep


def raw(A, b, m, keep, v_max, basis=True):
    """The kernel on the rows as given with an explicit keep mask (the public call takes none: one level below it)."""
    be = batch._Backend(A)
    B, m_max, d = A.shape
    V, count, status = be.out((B, v_max, d)), be.out((B,), np.int32), be.out((B,), np.int32)
    bas = be.out((B, v_max, d), np.int32) if basis else None
    be.call("plp_extreme_batch", B, m_max, d, A, b, m, keep, v_max, V, count, bas, status)
    return V, count, bas, status


# ------------------------------------------------------------------------------------------ the host build, bit for bit
@pytest.mark.parametrize("m_max,d", [(2, 1), (5, 2), (17, 2), (64, 2), (16, 3), (33, 3), (64, 3), (12, 4), (32, 4), (64, 4)])
def test_kernel_equals_the_host_build(L, m_max, d):
    """reduce=False and an explicit keep mask against the host build: identical status, count and basis, V bit for bit.
    B in {1, 5, 257}; (64, 4), 635 376 candidates per polytope, at B = 5.  One round and many, candidate counts that are no
    multiple of 64, ragged m with zeroed padding, keep masks with holes, repeated rows.  CUDA tensors give the same bits."""
    for B in ((5,) if (m_max, d) == (64, 4) else (1, 5, 257)):
        A, b, m, keep = raw_batch(B, m_max, d, seed=97 * d + m_max + B)
        v_max = xh.vmax_for(d, m_max)
        wV, wc, wb, ws = xh.run(L, A, b, m, keep, v_max)
        V, count, bas, status = raw(A, b, m, keep, v_max)
        assert np.array_equal(status, ws) and np.array_equal(count, wc), (B, np.argwhere(count != wc)[:5])
        assert np.array_equal(bas, wb)
        assert same_bits(V, wV)
        assert (ws == xh.XS_OK).any() or m_max < d + 1
        if B != 5:
            At, bt, mt, kt = dev(A, b, m, keep.view(np.int64))
            Vt, ct, bt_, st = raw(At, bt, mt, kt, v_max, basis=(B == 1))
            assert Vt.is_cuda and same_bits(Vt.cpu().numpy(), wV)
            assert np.array_equal(ct.cpu().numpy(), wc) and np.array_equal(st.cpu().numpy(), ws)
        # the public call without reduce: every row live
        res = batch.extreme_batch(A, b, m=m, v_max=v_max, reduce=False, basis=True)
        wV, wc, wb, ws = xh.run(L, A, b, m, None, v_max)
        assert same_bits(res["V"], wV) and np.array_equal(res["basis"], wb)
        assert np.array_equal(res["count"], wc) and np.array_equal(res["status"], ws)


def test_overflow_keeps_the_first_vertices():
    cube = np.vstack([np.eye(3), -np.eye(3)])[None]
    one = np.ones((1, 6))
    full = batch.extreme_batch(cube, one, reduce=False, basis=True)
    assert full["status"][0] == batch.XS_OK and full["count"][0] == 8 and full["V"].shape == (1, 8, 3)
    cut = batch.extreme_batch(cube, one, v_max=3, reduce=False, basis=True)
    assert cut["status"][0] == batch.XS_OVERFLOW and cut["count"][0] == 3
    assert same_bits(cut["V"], full["V"][:, :3]) and np.array_equal(cut["basis"], full["basis"][:, :3])
    assert batch.extreme_batch(cube, one, v_max=8, reduce=False)["status"][0] == batch.XS_OK
    assert set(map(tuple, full["V"][0])) == {(x, y, z) for x in (-1.0, 1.0) for y in (-1.0, 1.0) for z in (-1.0, 1.0)}


def test_cap_sweep_equals_the_host_build(L):
    """Overflow reached in a LATER round of 64 (tests/cap_sweep.py; the host build's own sweep is in test_extreme_host.py):
    at every cap from 1 to the full count + 1 the kernel's list is the host build's bit for bit, for the member twice in
    one launch."""
    for A, b in cap_sweep.extreme_members():
        A2, b2 = np.stack([A, A]), np.stack([b, b])
        full = int(xh.run(L, A[None], b[None])[1][0])
        for k in range(1, full + 2):
            wV, wc, wb, ws = xh.run(L, A2, b2, v_max=k)
            V, count, bas, status = raw(A2, b2, None, None, k)
            assert np.array_equal(status, ws) and np.array_equal(count, wc), (k, count, status)
            assert np.array_equal(bas, wb) and same_bits(V, wV), k
            assert (ws == (xh.XS_OVERFLOW if k < full else xh.XS_OK)).all() and (wc == min(k, full)).all()


# ------------------------------------------------------------------------------------------ the fixture, reduce=True
@pytest.fixture(scope="module")
def fixture_runs():
    """The whole fixture through extreme_batch(reduce=True), one call per dimension, with numpy arrays and with CUDA
    tensors -> (cases, numpy results, tensor results as numpy); a result is (V, count, status) per case."""
    cases = xh.fixture()
    out_np, out_t = [None] * len(cases), [None] * len(cases)
    for d in (2, 3, 4):
        sel, A, b, m = xh.pack(cases, d)
        rn = batch.extreme_batch(A, b, m=m)
        At, bt, mt = dev(A, b, m)
        rt = batch.extreme_batch(At, bt, m=mt)
        assert rt["V"].is_cuda and rt["basis"] is None
        rt = {k: v.cpu().numpy() for k, v in rt.items() if v is not None}
        for k, i in enumerate(sel):
            out_np[i] = (rn["V"][k], rn["count"][k], rn["status"][k])
            out_t[i] = (rt["V"][k], rt["count"][k], rt["status"][k])
    return cases, out_np, out_t


def test_fixture_numpy_input(fixture_runs):
    cases, out_np, _ = fixture_runs
    xh.check_cases(cases, out_np, "extreme_batch, numpy")


def test_fixture_cuda_tensors_same_bits(fixture_runs):
    cases, out_np, out_t = fixture_runs
    xh.check_cases(cases, out_t, "extreme_batch, CUDA tensors")
    for (Vn, cn, sn), (Vt, ct, st) in zip(out_np, out_t):
        assert cn == ct and sn == st and same_bits(Vn, Vt)


def test_flat_and_unbounded_have_no_vertices(fixture_runs):
    cases, out_np, _ = fixture_runs
    seen = set()
    for V, count, status in out_np:
        seen.add(int(status))
        if status in (batch.XS_FLAT, batch.XS_UNBOUNDED):
            assert count == 0 and np.all(np.isnan(V))
        else:
            assert np.all(np.isfinite(V[:count])) and np.all(np.isnan(V[count:]))
    assert {batch.XS_OK, batch.XS_FLAT, batch.XS_UNBOUNDED} <= seen


# ------------------------------------------------------------------------------------------ the C ABI
def test_c_abi_host_pointer_entry(L):
    lib = _lib.load()
    ctx = _lib.context()
    p = lambda a: None if a is None else C.c_void_p(a.ctypes.data)   # noqa: E731
    A, b, m, keep = raw_batch(37, 16, 3, seed=5)
    v_max = xh.vmax_for(3, 16)
    wV, wc, wb, ws = xh.run(L, A, b, m, keep, v_max)
    V, bas = np.empty((37, v_max, 3)), np.empty((37, v_max, 3), np.int32)
    count, status = np.empty(37, np.int32), np.empty(37, np.int32)
    rc = lib.plp_extreme_batch(ctx.handle, 37, 16, 3, p(A), p(b), p(m), p(keep), v_max, p(V), p(count), p(bas), p(status))
    assert rc == 0
    assert same_bits(V, wV) and np.array_equal(bas, wb) and np.array_equal(count, wc) and np.array_equal(status, ws)
    # without m, keep and basis: every row of every polytope
    rc = lib.plp_extreme_batch(ctx.handle, 37, 16, 3, p(A), p(b), None, None, v_max, p(V), p(count), None, p(status))
    wV, wc, _, ws = xh.run(L, A, b, None, None, v_max)
    assert rc == 0 and same_bits(V, wV) and np.array_equal(count, wc) and np.array_equal(status, ws)
    # the envelope
    z, i4 = np.zeros(512), np.zeros(8, np.int32)
    assert lib.plp_extreme_batch(ctx.handle, 1, 4, 5, p(z), p(z), None, None, 4, p(z), p(i4), None, p(i4)) == _lib.PLP_EUNSUPPORTED
    assert b"d=5" in lib.plp_last_error()
    assert lib.plp_extreme_batch(ctx.handle, 1, 65, 3, p(z), p(z), None, None, 4, p(z), p(i4), None, p(i4)) == _lib.PLP_EUNSUPPORTED
    assert lib.plp_extreme_batch(ctx.handle, 1, 4, 3, p(z), p(z), None, None, 0, p(z), p(i4), None, p(i4)) == _lib.PLP_EINVAL
    assert lib.plp_extreme_batch(ctx.handle, 0, 4, 3, None, None, None, None, 4, None, None, None, None) == 0
    assert lib.plp_extreme_batch_dev(ctx.handle, None, 0, 4, 3, None, None, None, None, 4, None, None, None, None) == 0
    empty = batch.extreme_batch(np.zeros((0, 6, 3)), np.zeros((0, 6)))
    assert empty["V"].shape[0] == 0 and empty["count"].shape == (0,)
