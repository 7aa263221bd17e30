"""GPU: the kernels built on walk3 (polytope_amd/csrc/plp_lane_lp.hpp: second and third pass peeled, the active
rows fetched together) on the families the host A/B test runs (tests/lane_walk_cases.py): lanes that stall on a
facet or an edge (boxes, cubes), unbounded box LPs (prisms), ragged row counts, rows a hair apart -- in tiles where the
lanes of a wavefront are in DIFFERENT cases, which the one-lane host build cannot produce.  Every tile shape, 16 and 32 row
slots, the hand-back path, the mix kernel the benchmark times, and the stand-alone bounding boxes."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
pytestmark = pytest.mark.gpu

_SWITCHES = ("PLP_REDUCE_LANE", "PLP_REDUCE_LANE_GS", "PLP_REDUCE_LANE_MIX", "PLP_REDUCE_RETRY_ALL")
NPOLY = 53   # three full 16-polytope tiles and a ragged one
SHAPES = [(16, 3), (24, 3), (16, 2)]


@pytest.fixture(scope="module")
def pa():
    import polytope_amd as pa
    from polytope_amd import _lib
    assert _lib.available(), "libplp_hip.so did not load or no gfx950 device: the HIP path is mandatory"
    return pa


@pytest.fixture
def run(pa):
    import torch

    def go(A, b, m=None, **env):
        for k in _SWITCHES:
            os.environ.pop(k, None)
        os.environ.update({k: str(v) for k, v in env.items()})
        try:
            t = lambda v, dt=None: None if v is None else torch.as_tensor(np.ascontiguousarray(v, dtype=dt)).cuda()  # noqa: E731
            res = pa.reduce_batch(t(A), t(b), t(m, np.int32))
            torch.cuda.synchronize()
            return {k: v.cpu().numpy() for k, v in res.items()}
        finally:
            for k in _SWITCHES:
                os.environ.pop(k, None)
    return go


@pytest.fixture(scope="module")
def cases(oracle):
    """{(m, d): [(family, A, b, mrows, oracle results per polytope)]}, computed once"""
    from lane_walk_cases import families
    out = {}
    for (m, d) in SHAPES:
        out[(m, d)] = [(name, A, b, mr, [oracle.reduce(A[k, :mr[k]], b[k, :mr[k]]) for k in range(NPOLY)])
                       for name, A, b, mr in families(NPOLY, d, m=m, seed=7)]
    return out


def _check(res, want, lo=0):
    for k, o in enumerate(want):
        k += lo
        assert int(res["keep"][k]) == o["mask"] and int(res["flags"][k]) == o["flags"] and int(res["nlp"][k]) == o["nlp"], \
            (k, hex(int(res["keep"][k])), hex(o["mask"]), int(res["flags"][k]), o["flags"], int(res["nlp"][k]), o["nlp"])
        assert abs(res["r"][k] - o["r"]) <= 1e-9, (k, res["r"][k], o["r"])


# (32 row slots: 8 or 4 polytopes per wavefront)
@pytest.mark.parametrize("shape,gs", [(s, g) for s in SHAPES for g in (4, 8, 16) if not (s[0] > 16 and g == 4)])
def test_walk_families_equal_the_oracle_in_every_tile_shape(run, cases, shape, gs):
    for name, A, b, mr, want in cases[shape]:
        try:
            _check(run(A, b, mr, PLP_REDUCE_LANE=1, PLP_REDUCE_LANE_GS=gs), want)
        except AssertionError as e:
            raise AssertionError((shape, gs, name) + e.args)


def test_walk_families_when_every_polytope_is_handed_back(run, cases):
    for name, A, b, mr, want in cases[(16, 3)]:
        _check(run(A, b, mr, PLP_REDUCE_LANE=1, PLP_REDUCE_RETRY_ALL=1), want)


def test_the_mix_kernel_of_the_benchmark(run, oracle):
    """40 001 x (16,3): the smallest batch the plan gives to reduce_lane_mix_kernel<3,16,4,8> (tests/test_reduce_plan.py) --
    every bit equal to the same batch on 16-polytope tiles alone, both ends equal to the oracle."""
    from polytope_amd.synth import random_hpolytopes
    B, n = 40001, 1500
    A, b = random_hpolytopes(B, 16, 3, seed=40001)
    mix = run(A, b)
    gs4 = run(A, b, PLP_REDUCE_LANE_GS=4)
    for key in ("keep", "flags", "nlp", "r", "xc"):
        assert np.array_equal(mix[key].view(np.uint8), gs4[key].view(np.uint8)), key
    for lo in (0, B - n):
        R = oracle.reduce_batch(A[lo:lo + n], b[lo:lo + n])
        assert np.array_equal(mix["keep"][lo:lo + n].view(np.uint64), R["keep"]), lo
        assert np.array_equal(mix["flags"][lo:lo + n], R["flags"]) and np.array_equal(mix["nlp"][lo:lo + n], R["nlp"]), lo
        assert np.all(np.abs(mix["r"][lo:lo + n] - R["r"]) <= 1e-9), lo


def test_walk_families_bounding_boxes(pa, oracle, cases):
    """bbox_lane_kernel on the (16,3) families: where it settles a polytope (status 0) the box is the oracle's to 1e-9,
    -inf / +inf in the same places; it settles the random batch completely."""
    import torch
    for name, A, b, mr, _ in cases[(16, 3)]:
        t = lambda v: torch.as_tensor(np.ascontiguousarray(v)).cuda()  # noqa: E731
        got = {k: v.cpu().numpy() for k, v in pa.bbox_batch(t(A), t(b), t(mr)).items()}
        if name == "random":
            assert not np.any(got["status"]), name
        nset = 0
        for k in range(NPOLY):
            if got["status"][k] != 0:
                continue
            lb, ub, bad = oracle.bounding_box(A[k, :mr[k]], b[k, :mr[k]])
            assert bad == 0, (name, k)
            nset += 1
            for mine, want in ((got["lb"][k], lb.ravel()), (got["ub"][k], ub.ravel())):
                fin = np.isfinite(want)
                assert np.array_equal(np.isfinite(mine), fin) and np.array_equal(np.sign(mine[~fin]), np.sign(want[~fin])), (name, k)
                assert np.all(np.abs(mine[fin] - want[fin]) <= 1e-9 * np.maximum(1.0, np.abs(want[fin]))), (name, k, mine, want)
        assert nset >= 10, (name, nset)   # (the rest have no bounded ball: ragged polytopes of a few rows)
