"""GPU: envelope_batch / is_convex_batch (envelope_cross_kernel, one list entry per wavefront) -- the raw call against a
brute force that sends every (member, row, partner) stack through cheby_ball_batch, the public calls against the loop of
single calls and against the reference's verdicts (g25), poison in everything the kernel must not read or write, every
status beside healthy neighbours, the single call's answer for what is beyond the caps, and the caller's stream."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import envelope_host as EH  # noqa: E402
from conftest import load_golden  # noqa: E402

pytestmark = pytest.mark.gpu

ABS_TOL = 1e-7


@pytest.fixture(scope="module")
def hip():
    from polytope_amd import solvers
    old, solvers.default_solver = solvers.default_solver, "hip"
    yield
    solvers.default_solver = old


def _all_tests(A, b, mc, reg_off, mem_idx):
    """Every (w, j, ii) of the reference's loops with its stack."""
    out = []
    for p in range(len(reg_off) - 1):
        lo, hi = int(reg_off[p]), int(reg_off[p + 1])
        for w in range(lo, hi):
            own = EH.member_of(reg_off, mem_idx, w)
            for ii in range(int(mc[own])):
                for j in range(hi - lo):
                    if lo + j != w:
                        out.append(((w, j, ii), EH.stack_of(A, b, mc, EH.member_of(reg_off, mem_idx, lo + j), own, ii)))
    return out


def _batch_radii(stacks):
    """The radius of every stack as cheby_ball reads it, all through ONE cheby_ball_batch."""
    from polytope_amd import batch
    if not stacks:
        return np.zeros(0)
    lens = np.array([s.shape[0] for s in stacks], np.int32)
    d = stacks[0].shape[1] - 1
    A3, b3 = np.zeros((len(stacks), int(lens.max()), d)), np.zeros((len(stacks), int(lens.max())))
    for t, s in enumerate(stacks):
        A3[t, :lens[t]], b3[t, :lens[t]] = s[:, :-1], s[:, -1]
    out = batch.cheby_ball_batch(A3, b3, m=lens)
    return np.where((out["status"] == 0) & (out["r"] >= 0), out["r"], 0.0)


def _brute(A, b, mc, reg_off, mem_idx):
    tests = _all_tests(A, b, mc, reg_off, mem_idx)
    R = dict(zip([k for k, _ in tests], _batch_radii([s for _, s in tests])))
    outer, opened, nlp, _ = EH.brute_force(A, b, mc, reg_off, mem_idx, ABS_TOL, lambda w, j, ii, _s: R[(w, j, ii)])
    return outer, opened, nlp, np.array(list(R.values()))


def _regions(B, d, seed):
    """B regions of 2..5 members of max(3, d + 1)..12 rows: from d + 1 rows on a member is bounded, and so is every stack
    (an unbounded stack has no radius on the device: NaN, ENV_OPEN -- test_every_status_on_the_device has one)."""
    rng = np.random.default_rng(seed)
    return EH.lists_of([EH.random_region(rng, d, int(rng.integers(2, 6)), max(3, d + 1), 12) for _ in range(B)])


@pytest.mark.parametrize("d", [2, 3, 4, 8])
@pytest.mark.parametrize("B", [1, 3, 67])
def test_raw_call_equals_the_brute_force(hip, B, d):
    """Test 5: outer equal wherever status is ENV_OK, nlp at most the brute force's.  No brute-force radius lies in
    (abs_tol / 4, 4 abs_tol) -- asserted -- so no entry may be ENV_OPEN."""
    from polytope_amd import batch
    A, b, mc, reg_off = _regions(B, d, 1000 * d + B)
    outer, opened, nlp, R = _brute(A, b, mc, reg_off, None)
    assert not np.any((R > ABS_TOL / 4) & (R < 4 * ABS_TOL)) and not opened.any()
    got = batch.envelope_outer_batch(A, b, mc, reg_off, None, ABS_TOL)
    assert got["outer"].dtype == np.uint64 and got["outer"].shape == outer.shape
    assert np.all(got["status"] == EH.ENV_OK), np.nonzero(got["status"])[0]
    assert np.array_equal(got["outer"], outer)
    assert np.all(got["nlp"] <= nlp) and (B == 1 or int(got["nlp"].sum()) < int(nlp.sum()))
    print("B=%d d=%d: %d entries, %d LPs against the brute force's %d" % (B, d, len(outer), got["nlp"].sum(), nlp.sum()))
    # the same from CUDA tensors, with the lists spelled out
    import torch
    idx = np.arange(len(outer), dtype=np.int32)
    dev = [torch.as_tensor(a, device="cuda:0") for a in (A, b, mc, reg_off, idx)]
    res = batch.envelope_outer_batch(*dev, abs_tol=ABS_TOL)
    assert all(v.is_cuda for v in res.values())
    assert np.array_equal(res["outer"].cpu().numpy().view(np.uint64), outer)
    assert np.array_equal(res["nlp"].cpu().numpy(), got["nlp"]) and not res["status"].any()


def _g25_regions(pcm):
    g = load_golden("g25_convex_regions.npz")
    regs = []
    for k in range(len(g["d"])):
        d = int(g["d"][k])
        regs.append(pcm.Region([pcm.Polytope(g["A"][k, q, :g["m"][k, q], :d].copy(), g["b"][k, q, :g["m"][k, q]].copy(),
                                             normalize=False) for q in range(int(g["n"][k]))]))
    return g, regs


def _same_envelope(got, want, what):
    assert (got is None) == (want is None), what
    if want is None:
        return
    assert got.A.shape == want.A.shape, (what, got.A.shape, want.A.shape)
    assert EH.hb.same_bits(got.A, want.A) and EH.hb.same_bits(got.b, want.b), what
    if want.A.size:
        assert abs(float(got.chebR) - float(want.chebR)) <= 1e-12, what
        assert np.allclose(np.ravel(got.chebXc), np.ravel(want.chebXc), rtol=0, atol=1e-12), what


def test_public_calls_equal_the_loop_and_the_reference(hip):
    """Test 6: on the g25 regions is_convex_batch / envelope_batch equal the loop of single calls on 'hip' -- bools equal,
    the envelopes' A and b bitwise, chebR / chebXc to 1e-12 -- the bools are the reference's, and none of these regions
    was handed to the single call."""
    import polytope_amd
    import polytope_amd.polytope as pcm
    g, regs = _g25_regions(pcm)
    info = {}
    env = polytope_amd.envelope_batch(_g25_regions(pcm)[1], _info=info)
    assert info["routed"] == 0 and 0 < info["nlp"] < info["tests"]
    print("g25: %d regions, the kernel ran %d LPs of the reference's %d" % (len(regs), info["nlp"], info["tests"]))
    got = polytope_amd.is_convex_batch(regs)
    want = [pcm.is_convex(r) for r in _g25_regions(pcm)[1]]
    want_env = [pcm.envelope(r) for r in _g25_regions(pcm)[1]]
    for k in range(len(regs)):
        assert bool(got[k][0]) == bool(want[k][0]) == bool(g["convex"][k]), k
        _same_envelope(got[k][1], want[k][1], ("is_convex", k))
        _same_envelope(env[k], want_env[k], ("envelope", k))
        ref_rows = g["env_Ab"][k, :g["env_m"][k]]
        assert env[k].A.shape[0] == ref_rows.shape[0], k
        d = int(g["d"][k])
        assert ref_rows.shape[0] == 0 or np.allclose(np.c_[env[k].A, env[k].b], np.c_[ref_rows[:, :d], ref_rows[:, 4]], rtol=0, atol=1e-9), k


def test_shared_members_and_an_empty_list(hip):
    """Test 6, second part: regions that share member OBJECTS (one table entry, listed by several regions through mem_idx)
    and a region without members, a Polytope and an empty batch beside them."""
    import polytope_amd
    import polytope_amd.polytope as pcm

    def build():
        sq = [pcm.Polytope(*EH_square(c, h)) for c, h in (((0, 0), 1), ((2, 0), 1), ((0, 2), 1), ((0.5, 0.5), 2), ((2, 2), 1))]
        return [pcm.Region([sq[0], sq[1]]), pcm.Region([sq[0], sq[2]]), pcm.Region([sq[0], sq[1], sq[2], sq[4]]),
                pcm.Region([sq[3], sq[0]]), pcm.Region([sq[0], sq[4]]), pcm.Region([sq[0], sq[0]]), pcm.Region(), sq[1]]
    got, want = polytope_amd.is_convex_batch(build()), [pcm.is_convex(r) for r in build()]
    assert [bool(v[0]) for v in want] == [True, True, True, True, False, True, True, True]
    for k, (gk, wk) in enumerate(zip(got, want)):
        assert bool(gk[0]) == bool(wk[0]), k
        _same_envelope(gk[1], wk[1], k)
    genv, wenv = polytope_amd.envelope_batch(build()[:6]), [pcm.envelope(r) for r in build()[:6]]
    for k in range(6):
        _same_envelope(genv[k], wenv[k], k)
    assert polytope_amd.is_convex_batch([]) == [] and polytope_amd.envelope_batch([]) == []
    with pytest.raises(AttributeError):   # (what envelope() raises for a region without members)
        polytope_amd.envelope_batch([pcm.Region()])


def EH_square(c, h):
    a = np.array([[1.0, 0], [0, 1.0], [-1.0, 0], [0, -1.0]])
    return a, a @ np.array(c, dtype=float) + h


def _dev_call(A, b, mc, reg_off, mem_idx, outer, status, nlp, n_entries, skip=0):
    """plp_envelope_batch_dev on CUDA tensors as they are; the outputs start `skip` elements into their tensors."""
    import torch
    from polytope_amd import _lib
    lib, ctx = _lib.load(), _lib.context(0)
    p = lambda t, off=0: None if t is None else C.c_void_p(t.data_ptr() + off * t.element_size())   # noqa: E731
    rc = lib.plp_envelope_batch_dev(ctx.handle, C.c_void_p(torch.cuda.current_stream().cuda_stream), A.shape[0], A.shape[1],
                                    A.shape[2], p(A), p(b), p(mc), reg_off.shape[0] - 1, p(reg_off), n_entries, p(mem_idx),
                                    ABS_TOL, p(outer, skip), p(status, skip), p(nlp, skip))
    assert rc == 0, rc
    torch.cuda.synchronize()


@pytest.mark.parametrize("poison", [float("nan"), 1e300])
def test_padding_unlisted_members_and_neighbours(hip, poison):
    """Test 7: NaN / 1e300 in every row beyond mc[c] and in members no list names change nothing, and the call writes
    exactly its L outputs: the elements in front of and behind them keep their sentinel."""
    import torch
    from polytope_amd import batch
    A, b, mc, reg_off = _regions(5, 3, 77)
    Cn = len(mc)
    want = batch.envelope_outer_batch(A, b, mc, reg_off, None, ABS_TOL)
    assert not want["status"].any()
    # the table with two unlisted members in front and one behind, all poison; padding rows poison
    Ap, bp = np.full((Cn + 3, A.shape[1] + 2, 3), poison), np.full((Cn + 3, A.shape[1] + 2), poison)
    mcp = np.concatenate([[5, 64], mc, [70]]).astype(np.int32)
    for c in range(Cn):
        Ap[c + 2, :mc[c]], bp[c + 2, :mc[c]] = A[c, :mc[c]], b[c, :mc[c]]
    idx = (np.arange(Cn) + 2).astype(np.int32)
    got = batch.envelope_outer_batch(Ap, bp, mcp, reg_off, idx, ABS_TOL)
    for key in ("outer", "status", "nlp"):
        assert np.array_equal(got[key], want[key]), key
    dev = [torch.as_tensor(a, device="cuda:0") for a in (Ap, bp, mcp, reg_off, idx)]
    outer = torch.full((Cn + 8,), -7, dtype=torch.int64, device="cuda:0")
    status, nlp = (torch.full((Cn + 8,), -7, dtype=torch.int32, device="cuda:0") for _ in range(2))
    _dev_call(*dev, outer, status, nlp, Cn, skip=4)
    for t, key in ((outer, "outer"), (status, "status"), (nlp, "nlp")):
        h = t.cpu().numpy()
        assert np.all(h[:4] == -7) and np.all(h[Cn + 4:] == -7), key
        assert np.array_equal(h[4:Cn + 4].view(want[key].dtype), want[key]), key


def test_every_status_on_the_device(hip):
    """Test 8: ENV_OK, ENV_OPEN (a radius inside the band; an unbounded stack, whose LP has no verdict), ENV_UNSUPPORTED
    (a member of 64 rows, one without rows, an index outside the table, offsets that hold no entry) and a region of one
    member, each beside healthy neighbours whose outputs are what they are alone."""
    from polytope_amd import batch
    rng = np.random.default_rng(8)
    sq = lambda cx, cy, h=1.0: EH_square((cx, cy), h)   # noqa: E731
    wide = (sq(0, 0)[0], sq(0, 0)[1] + np.array([2.4e-7, 0, 0, 0]))        # [-1, 1 + 2.4e-7] x [-1, 1]
    half = (np.array([[1.0, 0]]), np.array([5.0]))                          # the half-plane x <= 5
    big64 = EH.random_member(rng, 2, 64, np.zeros(2), 1.0)
    big63 = EH.random_member(rng, 2, 63, np.zeros(2), 1.0)
    members = [sq(0, 0), sq(1, 0),          # 0, 1: healthy
               sq(0, 0), wide,              # 2, 3: row 0 of 2 is overlapped by a slab of radius 1.2e-7: in the band
               sq(0, 0), half,              # 4, 5: [x <= 5; -y <= -1] is a quadrant: the LP is unbounded
               sq(0, 0),                    # 6: alone
               big64, sq(0, 0),             # 7, 8
               big63, sq(0, 0),             # 9, 10
               sq(0, 0), sq(0, 1)]          # 11, 12: healthy
    A, b, mc = EH.pack(members)
    reg_off = np.array([0, 2, 4, 6, 7, 9, 11, 13], np.int32)
    got = batch.envelope_outer_batch(A, b, mc, reg_off, None, ABS_TOL)
    ok, op, un = EH.ENV_OK, EH.ENV_OPEN, EH.ENV_UNSUPPORTED
    assert got["status"].tolist() == [ok, ok, op, ok, op, ok, ok, un, un, ok, ok, ok, ok]
    assert got["outer"][[0, 1, 6, 11, 12]].tolist() == [15 - 1, 15 - 4, 15, 15 - 2, 15 - 8]
    assert got["outer"][2] == 15 and got["outer"][4] & 2 and got["nlp"][6] == 0
    assert got["outer"][7:9].tolist() == [0, 0] and got["nlp"][7:9].tolist() == [0, 0]
    assert got["outer"][10] == 0 or got["status"][10] == ok   # (the 63-row member runs: 64-row stacks)
    assert got["nlp"][10] >= 1 and got["nlp"][9] >= 63
    # a member without rows, an index outside the table, offsets that hold no entry: only the lists concerned
    idx = np.arange(13, dtype=np.int32)
    mc0 = mc.copy()
    mc0[1] = 0
    assert batch.envelope_outer_batch(A, b, mc0, reg_off, idx, ABS_TOL)["status"].tolist() == \
        [un, un, op, ok, op, ok, ok, un, un, ok, ok, ok, ok]
    for bad in (13, -1, 1 << 30):
        idx2 = idx.copy()
        idx2[12] = bad
        res = batch.envelope_outer_batch(A, b, mc, reg_off, idx2, ABS_TOL)
        assert res["status"].tolist() == [ok, ok, op, ok, op, ok, ok, un, un, ok, ok, un, un]
        assert res["outer"][:2].tolist() == [15 - 1, 15 - 4]
    off2 = np.array([0, 2, 4, 6, 7, 9, 11, 10], np.int32)   # decreasing at the end: no pair of offsets holds entries 11, 12
    res = batch.envelope_outer_batch(A, b, mc, off2, idx, ABS_TOL)
    assert res["status"][11:].tolist() == [un, un] and res["status"][:2].tolist() == [ok, ok]
    off3 = np.array([2, 2, 4, 6, 7, 9, 11, 20], np.int32)   # starts above entry 0, ends beyond the list
    res = batch.envelope_outer_batch(A, b, mc, off3, idx, ABS_TOL)
    assert res["status"].tolist() == [un, un, op, ok, op, ok, ok, un, un, ok, ok, un, un]


def test_beyond_the_caps_is_the_single_calls_answer(hip):
    """Test 9: a region with a 64-row member and one in d = 9 come back as is_convex() / envelope() answer them, beside
    regions the kernel takes; and an ENV_OPEN region (a slab of radius 1.2e-7 beyond a facet) goes the same way."""
    import polytope_amd
    import polytope_amd.polytope as pcm

    def build():
        big = EH.random_member(np.random.default_rng(90), 2, 64, np.zeros(2), 1.0)
        box9 = pcm.box2poly([[0.0, 1.0]] * 9)
        box9b = pcm.box2poly([[1.0, 2.0]] + [[0.0, 1.0]] * 8)
        wide = (EH_square((0, 0), 1)[0], EH_square((0, 0), 1)[1] + np.array([2.4e-7, 0, 0, 0]))
        return [pcm.Region([pcm.Polytope(*EH_square((0, 0), 1)), pcm.Polytope(*EH_square((2, 0), 1))]),
                pcm.Region([pcm.Polytope(*big), pcm.Polytope(*EH_square((0, 0), 0.1))]),
                pcm.Region([box9, box9b]),
                pcm.Region([pcm.Polytope(*EH_square((0, 0), 1)), pcm.Polytope(*wide)]),
                pcm.Region([pcm.Polytope(*EH_square((0, 0), 1)), pcm.Polytope(*EH_square((0, 2), 1))])]
    info = {}
    genv = polytope_amd.envelope_batch(build(), _info=info)
    assert info["routed"] == 1   # (the slab; the 64-row member and d = 9 never reach the kernel)
    got, want, wenv = polytope_amd.is_convex_batch(build()), [pcm.is_convex(r) for r in build()], [pcm.envelope(r) for r in build()]
    assert bool(want[0][0]) and bool(want[2][0]) and bool(want[4][0])
    for k in range(5):
        assert bool(got[k][0]) == bool(want[k][0]), k
        _same_envelope(got[k][1], want[k][1], k)
        _same_envelope(genv[k], wenv[k], k)


def test_the_call_runs_on_the_callers_stream(hip):
    """Test 10: CUDA tensors in, on a stream of its own.  The tensors hold a decoy batch; on the stream: a delay, the copy
    of the real batch into the tensors, the call, clones of the outputs; only that stream is synchronised.  The masks are
    the real batch's -- a launch that went to the default stream would have answered for the decoy."""
    import torch
    from polytope_amd import batch
    import test_streams_gpu as TSG
    real = _regions(6, 3, 5)
    rng = np.random.default_rng(6)
    A, b, mc, reg_off = real
    decoy_b = b + rng.uniform(0.3, 0.6, b.shape) * (np.arange(b.shape[1])[None, :] < mc[:, None])
    want, other = (batch.envelope_outer_batch(A, bb, mc, reg_off, None, ABS_TOL) for bb in (b, decoy_b))
    assert not np.array_equal(want["outer"], other["outer"])
    live = [torch.as_tensor(a, device="cuda:0") for a in (A, decoy_b, mc, reg_off)]
    src_b = torch.as_tensor(b, device="cuda:0")
    warm = batch.envelope_outer_batch(*live, abs_tol=ABS_TOL)
    torch.cuda.synchronize()
    assert np.array_equal(warm["outer"].cpu().numpy().view(np.uint64), other["outer"])
    P = TSG.Prepared()
    P.torch, P.delay, P.probe = torch, TSG.Delay(torch), torch.zeros(1, device="cuda:0")
    P.delay.ms = 20.0
    s = TSG.stream_apart_from(P, torch.cuda.default_stream())
    with torch.cuda.stream(s):
        P.delay()
        live[1].copy_(src_b)
        res = batch.envelope_outer_batch(*live, abs_tol=ABS_TOL)
        clones = {k: v.clone() for k, v in res.items()}
    s.synchronize()
    assert all(v.is_cuda for v in res.values())
    assert np.array_equal(clones["outer"].cpu().numpy().view(np.uint64), want["outer"])
    assert np.array_equal(clones["nlp"].cpu().numpy(), want["nlp"]) and not clones["status"].cpu().numpy().any()
