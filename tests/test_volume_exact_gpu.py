"""GPU: volume_exact_kernel (csrc/plp_volume_exact.hip) through the C ABI and batch.volume_exact_batch, against the host
build of the same source (tests/cabi/volume_exact_host.cpp: volume, area and status bit for bit), under the packed-table
contract of tests/test_batch_contract_gpu.py (padding, order, batch size and repetition change no bit) and, through the
public call with reduce=True, against the reference (tests/golden/g30_volume_exact.npz; the comparison and the cap on misses
are those of tests/test_volume_exact_host.py, tests/volume_exact_host.py: check_cases)."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from polytope_amd import _lib, batch  # noqa: E402
import contract_cases as cc  # noqa: E402
import volume_exact_host as vh  # noqa: E402
from test_batch_contract_gpu import Case, Fresh, check_members, check_padding  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def L(tmp_path_factory):
    return vh.build(tmp_path_factory.mktemp("volume_exact_host"))


@pytest.fixture(scope="module")
def cases():
    return vh.fixture()


def dev(*arrays):
    import torch
    return [a if not isinstance(a, np.ndarray) else torch.as_tensor(a.view(np.int64) if a.dtype == np.uint64 else a).to("cuda:0")
            for a in arrays]


def raw(A, b, m=None, keep=None, xc=None, scale=None, areas=True):
    """The kernel on the rows as given (one level below the public call, which takes no keep word); every output is
    filled with a byte pattern first."""
    be = Fresh(A)
    B, m_max, d = A.shape
    res = dict(volume=be.out((B,)), area=be.out((B, m_max)) if areas else None, status=be.out((B,), np.int32))
    be.call("plp_vol_exact_batch", B, m_max, d, A, b, m, keep, xc, scale, res["volume"], res["area"], res["status"])
    return res


def host(L, A, b, m=None, keep=None, xc=None, scale=None, areas=True):
    vol, area, status = vh.run(L, A, b, m, keep, xc, scale, areas)
    return dict(volume=vol, area=area, status=status)


def assert_bits(got, want, what):
    for k, w in want.items():
        if w is None:
            assert got[k] is None
            continue
        g = got[k].cpu().numpy() if hasattr(got[k], "cpu") else got[k]
        assert cc.same_bits(g, w), (what, k, np.argwhere(np.asarray(g) != np.asarray(w))[:4].tolist())


def both_forms(L, args, what):
    """Host pointers and device pointers against the host build -> the host build's result."""
    want = host(L, **args)
    assert_bits(raw(**args), want, (what, "host pointers"))
    names = list(args)
    targs = dict(zip(names, dev(*[args[k] for k in names])))
    got = raw(**targs)
    assert got["volume"].is_cuda
    assert_bits(got, want, (what, "device pointers"))
    return want


def special_members(d, m_max, seed):
    """cc.mixed_rows at B = 257 (member 1 has no rows, member 2 has d: unbounded, member 3 is empty, member 4 flat) with, in
    addition: member 5 an infeasible zero row, member 6 a prism without its ends (d >= 2), member 7 fewer than d + 1 rows,
    member 8 every row twice."""
    A, b, m = cc.mixed_rows(257, m_max, d, seed)
    A[5, 1], b[5, 1] = 0.0, -1.0
    if d >= 2 and m_max >= 2 * d:
        rows = [k for k in range(2 * d) if k % d != d - 1]
        A[6], b[6] = 0.0, 0.0
        A[6, :len(rows)], b[6, :len(rows)], m[6] = A[0, rows], 3.0, len(rows)
    A[7, d:], b[7, d:], m[7] = 0.0, 0.0, d
    h = m_max // 2
    A[8, h:2 * h], b[8, h:2 * h], m[8] = A[8, :h], b[8, :h], 2 * h
    return A, b, m


# ------------------------------------------------------------------------------------------ the host build, bit for bit
@pytest.mark.parametrize("d,m_max", [(2, 16), (2, 24), (2, 64), (3, 24), (3, 64), (4, 16), (4, 24), (4, 64)])
def test_fixture_rows_equal_the_host_build(L, cases, d, m_max):
    """The fixture's rows of one dimension as one packed batch, padded to m_max: every row live; a keep word with holes; a
    centre and a scale; without the areas.  Volume, area and status bit for bit, host pointers and device pointers."""
    sel, A, b, m = vh.pack(cases, d, m_max)
    rng = np.random.default_rng(7 * d + m_max)
    keep = cc.keep_words(rng, len(sel), 2 * d)
    xc, scale = 0.1 * rng.standard_normal((len(sel), d)), np.exp(rng.uniform(-1, 1, len(sel)))
    want = both_forms(L, dict(A=A, b=b, m=m), "every row")
    assert (want["status"] == vh.VS_OK).sum() > len(sel) // 2 and np.all(want["area"][:, int(m.max()):] == 0.0)
    both_forms(L, dict(A=A, b=b, m=m, keep=keep), "keep")
    moved = both_forms(L, dict(A=A, b=b, m=m, xc=xc, scale=scale), "xc and scale")
    # (rows 1e-9 rad apart cross 1e-6 of the extent from where they would cross exactly: the dup family is left out here)
    ok = (want["status"] == vh.VS_OK) & (want["volume"] > 1e-6) & np.array([cases[i]["family"] != "dup" for i in sel])
    assert np.allclose(moved["volume"][ok], want["volume"][ok], rtol=1e-9, atol=0) and np.array_equal(moved["status"], want["status"])
    noar = both_forms(L, dict(A=A, b=b, m=m, areas=False), "no areas")
    assert cc.same_bits(noar["volume"], want["volume"])


@pytest.mark.parametrize("d,m_max", [(1, 2), (1, 9), (2, 5), (2, 16), (3, 7), (3, 16), (4, 9), (4, 16)])
def test_special_members_equal_the_host_build(L, d, m_max):
    """B = 257 and B = 1: m[p] = 0 and m[p] < d + 1, an infeasible zero row, an empty and a flat member, a prism without
    its ends, every row twice; one round of chains (few rows) and many."""
    A, b, m = special_members(d, m_max, seed=31 * d + m_max)
    keep = cc.keep_words(np.random.default_rng(d), 257, 2 * d)
    want = both_forms(L, dict(A=A, b=b, m=m), "B = 257")
    st, vol = want["status"], want["volume"]
    assert st[1] == vh.VS_UNBOUNDED and vol[1] == math.inf and st[5] == vh.VS_EMPTY and vol[5] == 0.0
    assert st[7] == vh.VS_UNBOUNDED and (st[2] == vh.VS_UNBOUNDED or d == 1)
    assert (st[3], vol[3]) == (vh.VS_OK, 0.0) and (m_max < 2 * d + 2 or (st[4] == vh.VS_OK and abs(vol[4]) <= 1e-12))
    if d >= 2 and m_max >= 2 * d:
        assert st[6] == vh.VS_UNBOUNDED and vol[6] == math.inf
    assert st[0] == vh.VS_OK and vol[0] > 0 and st[8] == (vh.VS_OK if m_max // 2 >= 2 * d else vh.VS_UNBOUNDED)
    both_forms(L, dict(A=A, b=b, m=m, keep=keep), "B = 257, keep")
    both_forms(L, dict(A=A, b=b), "B = 257, m = NULL")
    for p in (0, 6, 8):
        one = dict(A=A[p:p + 1].copy(), b=b[p:p + 1].copy(), m=m[p:p + 1].copy())
        alone = both_forms(L, one, "B = 1")
        assert cc.same_bits(alone["volume"], want["volume"][p:p + 1]) and cc.same_bits(alone["area"], want["area"][p:p + 1])


def test_closed_forms_on_the_device(L):
    for name, A, b, V in vh.closed_forms():
        res = raw(A[None].copy(), b[None].copy())
        assert res["status"][0] == vh.VS_OK and abs(res["volume"][0] - V) <= 1e-13 * V, (name, res["volume"][0])
        assert cc.same_bits(res["volume"], vh.run(L, A[None], b[None])[0])


# ------------------------------------------------------------------------------------------ the packed-table contract
@pytest.mark.parametrize("d,m_max", [(2, 12), (3, 16), (3, 24), (4, 16)])
def test_padding_and_members(d, m_max):
    """Outputs pre-filled with a byte pattern; NaN / 1e300 / answer-changing finite rows beyond m[p] and under clear keep bits
    change no output bit; the batch reversed and rolled by 3 gives the same bits, permuted; member p alone equals member p
    inside B = 257; two identical calls give identical bits."""
    A, b, m = special_members(d, m_max, seed=11 * d + m_max)
    rng = np.random.default_rng(d + m_max)
    for kp in (None, cc.keep_words(rng, 257, 2 * d)):
        args = dict(A=A, b=b, m=m, keep=kp) if kp is not None else dict(A=A, b=b, m=m)
        case = Case("volume_exact %s" % ("keep" if kp is not None else "all rows"), raw, args,
                    [(("A", "b"), "m", None if kp is None else "keep", "rows")], ("A", "b", "m") + (("keep",) if kp is not None else ()))
        want = check_padding(case)
        assert not np.any(want["volume"].view(np.uint64) == 0xA5A5A5A5A5A5A5A5)
        assert not np.any(want["area"].view(np.uint64) == 0xA5A5A5A5A5A5A5A5)
        check_members(case, want, alone=(0, 1, 5, 6, 100))


# ------------------------------------------------------------------------------------------ the fixture, reduce=True
@pytest.fixture(scope="module")
def fixture_runs(cases):
    """The whole fixture through volume_exact_batch(reduce=True), one call per dimension, with numpy arrays and with CUDA
    tensors -> (numpy results, tensor results as numpy, per case (volume, status, area, rows))."""
    out_np, out_t = [None] * len(cases), [None] * len(cases)
    for d in (2, 3, 4):
        sel, A, b, m = vh.pack(cases, d)
        rn = batch.volume_exact_batch(A, b, m=m)
        At, bt, mt = dev(A, b, m)
        rt = batch.volume_exact_batch(At, bt, m=mt)
        assert rt["volume"].is_cuda and rt["area"].is_cuda
        rt = {k: v.cpu().numpy() for k, v in rt.items()}
        for k, i in enumerate(sel):
            out_np[i] = (rn["volume"][k], rn["status"][k], rn["area"][k])
            out_t[i] = (rt["volume"][k], rt["status"][k], rt["area"][k])
    return out_np, out_t


def test_fixture_numpy_input(cases, fixture_runs):
    out_np, _ = fixture_runs
    vh.check_cases(cases, [(v, s) for v, s, _ in out_np], "volume_exact_batch, numpy")
    seen = set()
    for c, (vol, status, area) in zip(cases, out_np):
        seen.add(int(status))
        m = len(c["b"])
        assert np.all(area[m:] == 0.0)
        if status == batch.VS_OK:   # a closed surface: the areas weighted by their unit normals cancel
            un = c["A"] / np.linalg.norm(c["A"], axis=1)[:, None]
            assert np.abs(area[:m] @ un).max() <= 1e-12 * area.sum(), c["index"]
        else:
            assert np.all(area == 0.0) and vol == (0.0 if status == batch.VS_FLAT else math.inf)
    assert {batch.VS_OK, batch.VS_FLAT, batch.VS_UNBOUNDED} <= seen


def test_fixture_cuda_tensors_same_bits(cases, fixture_runs):
    out_np, out_t = fixture_runs
    vh.check_cases(cases, [(v, s) for v, s, _ in out_t], "volume_exact_batch, CUDA tensors")
    for (vn, sn, an), (vt, st, at) in zip(out_np, out_t):
        assert sn == st and cc.same_bits(np.float64(vn), np.float64(vt)) and cc.same_bits(an, at)


def test_public_call_without_reduce_and_one_polytope(L, cases, fixture_runs):
    import polytope_amd as pa
    sel, A, b, m = vh.pack(cases, 3)
    res = batch.volume_exact_batch(A, b, m=m, reduce=False)
    assert_bits(res, host(L, A, b, m), "reduce=False")
    res = batch.volume_exact_batch(A, b, m=m, reduce=False, areas=False)
    assert res["area"] is None and cc.same_bits(res["volume"], host(L, A, b, m)["volume"])
    out_np, _ = fixture_runs
    for i in sel[::9]:
        P = pa.Polytope(cases[i]["A"].copy(), cases[i]["b"].copy())
        v = pa.volume_exact(P)
        # (the constructor normalises the rows again: the last bits of the rows, and of the volume, may move)
        alone = batch.volume_exact_batch(np.asarray(P.A)[None], np.asarray(P.b)[None])["volume"][0]
        assert isinstance(v, float) and cc.same_bits(np.float64(v), np.float64(alone)) and P._volume is None
        assert not np.isfinite(v) or abs(v - out_np[i][0]) <= 1e-12 * max(1.0, abs(v))
    box = pa.box2poly([[0.0, 1.0], [0.0, 2.0]])
    assert pa.volume_exact(box) == 2.0
    with pytest.raises(Exception, match="regions"):
        pa.volume_exact(pa.Region([box, box]))


# ------------------------------------------------------------------------------------------ the C ABI
def test_c_abi_argument_checks():
    lib = _lib.load()
    ctx = _lib.context()
    p = lambda a: None if a is None else C.c_void_p(a.ctypes.data)   # noqa: E731
    z, i4 = np.zeros(512), np.zeros(8, np.int32)
    call = lib.plp_vol_exact_batch
    assert call(ctx.handle, 1, 4, 5, p(z), p(z), None, None, None, None, p(z), p(z), p(i4)) == _lib.PLP_EUNSUPPORTED == 2
    assert b"d=5" in lib.plp_last_error()
    assert call(ctx.handle, 1, 4, 0, p(z), p(z), None, None, None, None, p(z), p(z), p(i4)) == _lib.PLP_EUNSUPPORTED
    assert call(ctx.handle, 1, 65, 3, p(z), p(z), None, None, None, None, p(z), p(z), p(i4)) == _lib.PLP_EUNSUPPORTED
    assert lib.plp_vol_exact_batch_dev(ctx.handle, None, 1, 65, 3, p(z), p(z), None, None, None, None, p(z), p(z), p(i4)) == 2
    assert call(ctx.handle, 1, 4, 3, p(z), p(z), None, None, None, None, None, p(z), p(i4)) == _lib.PLP_EINVAL
    assert call(ctx.handle, 0, 4, 3, None, None, None, None, None, None, None, None, None) == 0
    assert lib.plp_vol_exact_batch_dev(ctx.handle, None, 0, 4, 3, None, None, None, None, None, None, None, None, None) == 0
    # m, keep, xc, scale and area may all be NULL
    A, b = vh.cube(3, 0.75)
    vol, st = np.zeros(1), np.full(1, -1, np.int32)
    assert call(ctx.handle, 1, 6, 3, p(np.ascontiguousarray(A)), p(b), None, None, None, None, p(vol), None, p(st)) == 0
    assert (vol[0], st[0]) == (3.375, 0)
