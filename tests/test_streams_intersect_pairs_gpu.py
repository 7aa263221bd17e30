"""GPU: intersect_pairs / intersect_cross_sparse on non-default streams (the other tests of these calls:
tests/test_intersect_pairs_gpu.py).  A file of its own that sorts behind tests/test_streams_gpu.py, for the reason
tests/test_streams_pairs_sparse_gpu.py gives: the context keeps per-stream scratch for 16 streams, and a test that brings a new
stream runs after the timed controls of that file."""
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


def _tables(torch, dev):
    A1, b1, _ = H.grid_cells((4, 4, 3))
    A2, b2, _ = H.grid_cells((4, 4, 3), origin=(0.5, 0.5, 0.5))
    At, bt = _dev(torch, dev, np.concatenate([A1, A2]), np.concatenate([b1, b2]))
    pairs = np.array([(i, 48 + j) for i in range(48) for j in range(48)], dtype=np.int32)
    return At, bt, _dev(torch, dev, pairs)[0]


def _equal(torch, got, want, keys):
    def bits(t):   # (xc is NaN for an empty intersection: compare the bits)
        return t.view(torch.int64) if t.dtype == torch.float64 else t
    return all(torch.equal(bits(got[k]), bits(want[k])) for k in keys)


def test_non_default_stream(env):
    torch, pa, dev = env
    At, bt, pt = _tables(torch, dev)
    want = pa.batch.intersect_pairs(At, bt, pt, chunk=1000)
    want_x = pa.intersect_cross_sparse(At, bt, 48)
    torch.cuda.synchronize()
    st = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(st):
        got = pa.batch.intersect_pairs(At, bt, pt, chunk=1000)
        got_x = pa.intersect_cross_sparse(At, bt, 48, max_candidates=100)
    st.synchronize()
    assert _equal(torch, got, want, ("keep", "flags", "nlp", "ms", "m", "A", "b", "r", "xc"))
    assert _equal(torch, got_x, want_x, ("pairs", "m", "A", "b")) and int(got_x["pairs"].shape[0]) > 0


def test_two_streams_interleaved(env):
    """Calls issued alternately on two streams, chunked so that each call reuses its stream's scratch several times: the
    scratch is per stream, so neither call sees the other's stacks."""
    torch, pa, dev = env
    At, bt, pt = _tables(torch, dev)
    half = int(pt.shape[0]) // 2
    lists = (pt[:half].contiguous(), pt[half:].contiguous())
    want = [pa.batch.intersect_pairs(At, bt, p, chunk=300) for p in lists]
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream(device=dev), torch.cuda.Stream(device=dev)]
    got = [[], []]
    for _ in range(3):
        for s in (0, 1):
            with torch.cuda.stream(streams[s]):
                got[s].append(pa.batch.intersect_pairs(At, bt, lists[s], chunk=300))
    for st in streams:
        st.synchronize()
    for s in (0, 1):
        for g in got[s]:
            assert _equal(torch, g, want[s], ("keep", "flags", "nlp", "ms", "m", "A", "b", "r", "xc"))
