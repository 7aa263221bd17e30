"""GPU: the ratio-test row loop of the lane kernels (lane::ratio_rows, plp_lane_lp.hpp) at the smallest inputs that take each
of its paths through reduce_lane_kernel / bbox_lane_kernel: B = 1 runs the whole F2 list in quads, B = 3 in pairs, B = 17 is a
full 16-polytope tile plus one polytope, B = 33 two full tiles (the second tile's F2 list on single lanes); 16 and 32 row
slots, d = 1 .. 4, every tile shape (LPs on single lanes, pairs and quads: a lane's share of the rows starts at i0 != 0).
Verdicts equal to the oracle's, r within 1e-9, and on random rows every tile shape bit for bit the same."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
pytestmark = pytest.mark.gpu

_SWITCHES = ("PLP_REDUCE_LANE", "PLP_REDUCE_LANE_GS", "PLP_REDUCE_LANE_MIX", "PLP_REDUCE_RETRY_ALL")
SHAPES = [(16, 3), (5, 3), (16, 2), (16, 1), (17, 3), (32, 3), (12, 4), (20, 4)]
BATCHES = (1, 3, 17, 33)


@pytest.fixture(scope="module")
def pa():
    import polytope_amd as pa
    from polytope_amd import _lib
    assert _lib.available(), "libplp_hip.so did not load or no gfx950 device: the HIP path is mandatory"
    return pa


def _reduce(pa, A, b, **env):
    import torch
    for k in _SWITCHES:
        os.environ.pop(k, None)
    os.environ.update({k: str(v) for k, v in env.items()})
    try:
        res = pa.reduce_batch(torch.tensor(A).cuda(), torch.tensor(b).cuda())   # (copies: the shared cases are read-only)
        torch.cuda.synchronize()
        return {k: v.cpu().numpy() for k, v in res.items()}
    finally:
        for k in _SWITCHES:
            os.environ.pop(k, None)


def _spoil(A, b, rng):
    """duplicated, shifted-parallel and infeasible rows (as tests/test_reduce_lane_gpu.py), dense enough for 1 .. 33 polytopes"""
    B, m, _ = A.shape
    for k in range(0, B, 2):
        j = int(rng.integers(m))
        A[k, (j + 1) % m] = A[k, j]
        b[k, (j + 1) % m] = b[k, j] + rng.choice([0.0, 0.05])
    for k in range(2, B, 7):
        b[k, 0] = -4.0


@pytest.fixture(scope="module")
def cases(oracle):
    """(m, d, B, spoiled) -> (A, b, the oracle's reduce): computed once, shared, never written to"""
    from polytope_amd.synth import random_hpolytopes
    rng = np.random.default_rng(29)
    out = {}
    for (m, d) in SHAPES:
        for B in BATCHES:
            A, b = random_hpolytopes(B, m, d, seed=1000 * m + 10 * d + B)
            for spoiled in (False, True):
                if spoiled:
                    A, b = A.copy(), b.copy()
                    _spoil(A, b, rng)
                for v in (A, b):
                    v.setflags(write=False)
                out[(m, d, B, spoiled)] = (A, b, oracle.reduce_batch(A, b))
    return out


@pytest.mark.parametrize("m,d", SHAPES)
def test_row_loop_paths_of_reduce(pa, cases, m, d):
    lane = {"PLP_REDUCE_LANE": 1} if d == 4 else {}
    # (17..32 rows take 32 row slots, at most four per lane: 8 or 16 lanes per polytope)
    shapes = [{}] + [{"PLP_REDUCE_LANE_GS": gs} for gs in (4, 8, 16) if m <= 16 or gs >= 8]
    for B in BATCHES:
        for spoiled in (False, True):
            A, b, R = cases[(m, d, B, spoiled)]
            got = []
            for env in shapes:
                res = _reduce(pa, A, b, **lane, **env)
                what = (m, d, B, spoiled, env)
                assert np.array_equal(res["keep"].view(np.uint64), R["keep"]), what
                assert np.array_equal(res["flags"], R["flags"]) and np.array_equal(res["nlp"], R["nlp"]), what
                assert bool(np.all(np.abs(res["r"] - R["r"]) <= 1e-9)), what
                got.append(res)
            if not spoiled:   # random rows: no ties in F1's ratio test, every bit of every tile shape the same
                for res, env in zip(got[1:], shapes[1:]):
                    for key in ("keep", "flags", "nlp", "r", "xc"):
                        assert np.array_equal(res[key].view(np.uint8), got[0][key].view(np.uint8)), (m, d, B, env, key)


@pytest.mark.parametrize("m,d", [(16, 3), (24, 2)])
def test_row_loop_paths_of_bbox(pa, m, d):
    import torch
    from polytope_amd.synth import random_hpolytopes
    rng = np.random.default_rng(5)
    for B in (1, 17, 33):
        A, b = random_hpolytopes(B, m, d, seed=77 * m + B)
        b = b + np.einsum("bij,bj->bi", A, rng.standard_normal((B, d)))   # boxes away from the origin
        for spoiled in (False, True):
            if spoiled:
                _spoil(A, b, rng)
            At, bt = torch.as_tensor(A).cuda(), torch.as_tensor(b).cuda()
            out = {}
            for sw in (None, "0"):
                os.environ.pop("PLP_BBOX_LANE", None)
                if sw is not None:
                    os.environ["PLP_BBOX_LANE"] = sw
                try:
                    out[sw] = {k: v.cpu().numpy() for k, v in pa.bbox_batch(At, bt).items()}
                finally:
                    os.environ.pop("PLP_BBOX_LANE", None)
            ln, g = out[None], out["0"]
            assert np.array_equal(ln["status"], g["status"]), (m, d, B, spoiled)
            both = (g["status"] == 0) & (ln["status"] == 0)
            assert spoiled or both.all(), (m, d, B)
            for key in ("lb", "ub"):
                x, y = g[key][both], ln[key][both]
                assert np.array_equal(np.isinf(x), np.isinf(y)) and np.array_equal(np.sign(x[np.isinf(x)]), np.sign(y[np.isinf(y)]))
                fin = np.isfinite(x)
                assert np.all(np.abs(x[fin] - y[fin]) <= 1e-9), (m, d, B, spoiled, key)
