"""GPU: the sparse pair screens on a non-default stream (the other tests of these calls: tests/test_pairs_sparse_gpu.py).
A file of its own that sorts behind tests/test_streams_gpu.py: the context keeps per-stream scratch for 16 streams and empties
the tables when a seventeenth comes (a device synchronise), and the controls of that file are timed against the streams the
process has seen before them -- a test that brings a new stream runs after it."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import box_pairs_host as H  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env():
    import torch
    import polytope_amd as pa
    assert torch.cuda.is_available()
    return torch, pa, torch.device("cuda:0")


def _dev(torch, dev, *arrays):
    return [None if a is None else torch.as_tensor(np.ascontiguousarray(a)).to(dev) for a in arrays]


def test_non_default_stream(env):
    torch, pa, dev = env
    A, b, _ = H.grid_cells((5, 5, 4))
    At, bt = _dev(torch, dev, A, b)
    want = pa.adjacent_pairs_sparse(At, bt)
    torch.cuda.synchronize()
    st = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(st):
        got = pa.adjacent_pairs_sparse(At, bt, max_candidates=100)
        got_ov = pa.overlap_cross_sparse(At, bt, 40)
        want_ov = torch.nonzero(pa.batch.overlap_cross(At, bt, 40)).to(torch.int32)
    st.synchronize()
    assert torch.equal(got["pairs"], want["pairs"]) and torch.equal(got_ov["pairs"], want_ov)
