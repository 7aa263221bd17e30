"""GPU: the lane kernels with the vertex round in walk3's general loop (polytope_amd/csrc/plp_lane_lp.hpp), at the smallest shapes at which a tile edge or a mode can go wrong: one polytope, one
short of / exactly / one over a 16-polytope tile, more than one block; every tile shape; 32 row slots; d = 1 and 2 embedded
in R^3; every polytope handed back; the smallest batch that launches the mix kernel; the stand-alone bounding boxes.  On
the families of tests/lane_walk_cases.py (random, ragged row counts, prisms, boxes / cubes, `dup`) the results are the
oracle's, and the centre and radius are, bit for bit, those of the lane-group kernels (PLP_REDUCE_LANE=0)."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
pytestmark = pytest.mark.gpu

_SWITCHES = ("PLP_REDUCE_LANE", "PLP_REDUCE_LANE_GS", "PLP_REDUCE_LANE_MIX", "PLP_REDUCE_RETRY_ALL", "PLP_BBOX_LANE")
# (rows, d) -> the largest batch; smaller ones are its leading polytopes
NMAX = {(16, 3): 65, (24, 3): 9, (16, 2): 17, (16, 1): 17}


@pytest.fixture(scope="module")
def pa():
    import polytope_amd as pa
    from polytope_amd import _lib
    assert _lib.available(), "libplp_hip.so did not load or no gfx950 device: the HIP path is mandatory"
    return pa


def _with_env(fn, env):
    for k in _SWITCHES:
        os.environ.pop(k, None)
    os.environ.update({k: str(v) for k, v in env.items()})
    try:
        return fn()
    finally:
        for k in _SWITCHES:
            os.environ.pop(k, None)


@pytest.fixture
def run(pa):
    import torch

    def go(A, b, m=None, **env):
        def call():
            t = lambda v, dt=None: None if v is None else torch.as_tensor(np.ascontiguousarray(v, dtype=dt)).cuda()  # noqa: E731
            res = pa.reduce_batch(t(A), t(b), t(m, np.int32))
            torch.cuda.synchronize()
            return {k: v.cpu().numpy() for k, v in res.items()}
        return _with_env(call, env)
    return go


@pytest.fixture(scope="module")
def cases(oracle):
    """{(m, d): [(family, A, b, mrows, oracle results per polytope)]}, computed once"""
    from lane_walk_cases import families
    out = {}
    for (m, d), n in NMAX.items():
        out[(m, d)] = [(name, A, b, mr, [oracle.reduce(A[k, :mr[k]], b[k, :mr[k]]) for k in range(n)])
                       for name, A, b, mr in families(n, d, m=m, seed=11)]
        assert [c[0] for c in out[(m, d)]] == ["random", "ragged", "prism", "box", "dup"]
    return out


def _check(res, want):
    assert len(res["keep"]) == len(want)
    for k, o in enumerate(want):
        assert int(res["keep"][k]) == o["mask"] and int(res["flags"][k]) == o["flags"] and int(res["nlp"][k]) == o["nlp"], \
            (k, hex(int(res["keep"][k])), hex(o["mask"]), int(res["flags"][k]), o["flags"], int(res["nlp"][k]), o["nlp"])
        assert abs(res["r"][k] - o["r"]) <= 1e-9, (k, res["r"][k], o["r"])


def _same_as_partner(res, ref):
    for key in ("r", "xc"):
        assert np.array_equal(res[key].view(np.uint64), ref[key].view(np.uint64)), key
    for key in ("keep", "flags", "nlp"):
        assert np.array_equal(res[key], ref[key]), key


def _all(run, cases, shape, B, **env):
    for name, A, b, mr, want in cases[shape]:
        try:
            res = run(A[:B], b[:B], mr[:B], PLP_REDUCE_LANE=1, **env)
            _check(res, want[:B])
            _same_as_partner(res, run(A[:B], b[:B], mr[:B], PLP_REDUCE_LANE=0))
        except AssertionError as e:
            raise AssertionError((shape, B, env, name) + e.args)


@pytest.mark.parametrize("gs", [4, 8, 16])
@pytest.mark.parametrize("B", [1, 15, 16, 17, 65])
def test_every_tile_shape_at_the_tile_edges(run, cases, B, gs):
    _all(run, cases, (16, 3), B, PLP_REDUCE_LANE_GS=gs)


def test_32_row_slots(run, cases):
    _all(run, cases, (24, 3), 9)


@pytest.mark.parametrize("shape", [(16, 2), (16, 1)])
def test_lower_dimensions_embedded(run, cases, shape):
    _all(run, cases, shape, 17)


def test_every_polytope_handed_back(run, cases):
    _all(run, cases, (16, 3), 17, PLP_REDUCE_RETRY_ALL=1)


def test_smallest_batch_of_the_mix_kernel(run, oracle):
    """40 016 x (16,3): past the 40 000 from which the plan launches reduce_lane_mix_kernel<3,16,4,8>
    (tests/test_reduce_plan.py)."""
    from polytope_amd.synth import random_hpolytopes
    B, n = 40016, 1000
    A, b = random_hpolytopes(B, 16, 3, seed=40016)
    mix = run(A, b)
    _same_as_partner(mix, run(A, b, PLP_REDUCE_LANE=0))
    for lo in (0, B - n):
        R = oracle.reduce_batch(A[lo:lo + n], b[lo:lo + n])
        assert np.array_equal(mix["keep"][lo:lo + n].view(np.uint64), R["keep"]), lo
        assert np.array_equal(mix["flags"][lo:lo + n], R["flags"]) and np.array_equal(mix["nlp"][lo:lo + n], R["nlp"]), lo
        assert np.all(np.abs(mix["r"][lo:lo + n] - R["r"]) <= 1e-9), lo


def test_bounding_boxes_equal_the_lane_group_kernel(pa, cases):
    """bbox_lane_kernel at (16,3) x 17 against PLP_BBOX_LANE=0: the same status, the same boxes to 1e-11."""
    import torch
    for name, A, b, mr, _ in cases[(16, 3)]:
        def call():
            t = lambda v: torch.as_tensor(np.ascontiguousarray(v)).cuda()  # noqa: E731
            got = pa.bbox_batch(t(A[:17]), t(b[:17]), t(mr[:17]))
            torch.cuda.synchronize()
            return {k: v.cpu().numpy() for k, v in got.items()}
        lane, grp = _with_env(call, {}), _with_env(call, {"PLP_BBOX_LANE": 0})
        assert np.array_equal(lane["status"], grp["status"]), name
        ok = lane["status"] == 0
        if name == "random":
            assert np.all(ok), name
        for key in ("lb", "ub"):
            x, y = lane[key][ok], grp[key][ok]
            fin = np.isfinite(y)
            assert np.array_equal(np.isfinite(x), fin) and np.array_equal(x[~fin], y[~fin]), (name, key)
            assert np.all(np.abs(x[fin] - y[fin]) <= 1e-11), (name, key, np.max(np.abs(x[fin] - y[fin])))
