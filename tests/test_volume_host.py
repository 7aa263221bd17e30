"""CPU: the arithmetic of the device volume (polytope_amd/csrc/plp_volume.hpp) in its host build -- numpy's PCG64 stream
bit for bit, jump-ahead against PCG64.advance, the sample-and-test loop against the reference's hit counts (g28) -- and the
argument handling of polytope_amd.batch.volume_batch that needs no device."""
import numpy as np
import pytest

from conftest import load_golden
import volume_host as vh

SEEDS = [0, 1, 2, 3, 7, 42, 255, 65536, 12345, 2 ** 31 - 1, 2 ** 32, 2 ** 53 + 1, 2 ** 63 - 25, 2 ** 63 - 1, 2 ** 63,
         2 ** 64 - 1, 2 ** 64,
         # the 128-bit kind np.random.SeedSequence().entropy gives, recorded
         0x9F3C2A7E5D1B48C60A1F2E3D4C5B6A79, 0x31D0B1F1A2C8E4F70918273645ABCDEF, 0xFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFF,
         0x8000000000000000000000000000000, 200289424572164523903456189732891733451, 52791567204618209786213409187623450981]
SHAPES = [(1, 50), (3, 3000), (16, 10000)]


@pytest.fixture(scope="module")
def L(tmp_path_factory):
    return vh.build(tmp_path_factory.mktemp("volume_host"))


def g28_cases():
    g = load_golden("g28_volume_batch.npz")
    out = []
    for k in range(int(g["n"])):
        r0, r1, c0, c1 = g["row_off"][k], g["row_off"][k + 1], g["dim_off"][k], g["dim_off"][k + 1]
        d = int(g["d"][k])
        ns = int(g["nsamples"][k])
        out.append(dict(A=None, k=k, d=d, m=int(g["m"][k]), ns=ns,
                        N=({1: 50, 2: 500, 3: 3000}.get(d, 10000)) if ns < 0 else ns, seed=int(g["seed"][k]),
                        vol=float(g["vol"][k]), hits=int(g["hits"][k]), lb=g["lb"][c0:c1], ub=g["ub"][c0:c1],
                        b=g["b"][r0:r1], family=str(g["family"][k])))
    # A is stored flat, case after case, m * d numbers each
    a_off = np.concatenate([[0], np.cumsum(g["m"] * g["d"])])
    for c in out:
        c["A"] = g["A"][a_off[c["k"]]:a_off[c["k"] + 1]].reshape(c["m"], c["d"])
    return out


def test_stream_equals_numpy(L):
    """Every double of default_rng(seed).random((n, N)), >= 20 seeds, the three shapes: bit for bit."""
    assert len(SEEDS) >= 20
    for seed in SEEDS:
        for n, N in SHAPES:
            ref = np.random.default_rng(seed).random((n, N))
            got = vh.stream(L, seed, n * N).reshape(n, N)
            assert np.array_equal(got.view(np.uint64), ref.view(np.uint64)), (seed, n, N)
        # element (i, j) is stream position i * N + j, reached directly
        rng = np.random.default_rng(5)
        pos = rng.integers(0, 16 * 10000, 200)
        assert np.array_equal(vh.at(L, seed, pos), ref.ravel()[pos]), seed


def test_advance_equals_numpy(L):
    """pcg64_advance (and pcg64_jump + pcg64_apply, the kernel's per-call constants) to 1000 positions up to 2^40 against
    np.random.PCG64(seed).advance(n)."""
    rng = np.random.default_rng(40)
    n = np.concatenate([[0, 1, 2, 255, 256, 257, 2 ** 31 - 1, 2 ** 32, 2 ** 40], rng.integers(0, 2 ** 40, 991)])
    assert n.size == 1000
    for seed in SEEDS[::4]:
        want = []
        for v in n:
            bg = np.random.PCG64(seed)
            bg.advance(int(v))
            want.append(bg.state["state"]["state"])
        assert vh.advance(L, seed, n, jump=False) == want, seed
        assert vh.advance(L, seed, n, jump=True) == want, seed
    # beyond 2^40: the full 64-bit range of the argument
    big = np.array([2 ** 63, 2 ** 64 - 1, 2 ** 50 + 12345], dtype=np.uint64)
    bgs = []
    for v in big:
        bg = np.random.PCG64(3)
        bg.advance(int(v))
        bgs.append(bg.state["state"]["state"])
    assert vh.advance(L, 3, big) == bgs and vh.advance(L, 3, big, jump=True) == bgs


def test_hits_equal_reference_g28(L):
    """The whole sample-and-test loop on g28, the reference's own boxes passed in: the reference's hit counts, and with
    them the reference's float."""
    cases = g28_cases()
    assert len(cases) >= 200
    assert {c["d"] for c in cases} == {1, 2, 3, 4, 5, 6, 7, 8, 12, 16}
    for c in cases:
        st, inc = vh.seed_state(c["seed"])
        h, fl = vh.hits(L, c["A"][None], c["b"][None], c["lb"][None], c["ub"][None], st[None], inc[None], c["N"])
        assert int(fl[0]) == 0
        assert int(h[0]) == c["hits"], (c["k"], c["family"], c["d"], c["N"])
        assert np.prod(c["ub"] - c["lb"]) * int(h[0]) / c["N"] == c["vol"], c["k"]


def test_hits_flags_and_padding(L):
    """A box that is not finite or a polytope without rows is flagged and not sampled; rows beyond m are not read."""
    A = np.zeros((3, 4, 2))
    b = np.zeros((3, 4))
    A[:, :4] = np.array([[1, 0], [-1, 0], [0, 1], [0, -1.0]])
    b[:, :4] = 1.0
    A[2, 2:] = 7.0   # padding of polytope 2 (m = 2): garbage that must not count
    lb = np.array([[-1, -1], [-np.inf, -1], [-2, -2.0]])
    ub = np.array([[1, 1], [1, 1], [2, 2.0]])
    st, inc = vh.seed_state(9)
    h, fl = vh.hits(L, A, b, lb, ub, np.tile(st, (3, 1)), np.tile(inc, (3, 1)), 1000, m=np.array([4, 4, 2], np.int32))
    assert list(fl) == [0, 1, 0] and h[0] == 1000 and h[1] == 0
    x = -2 + np.random.default_rng(9).random((2, 1000)) * 4
    assert h[2] == np.count_nonzero(np.abs(x[0]) < 1)
    h, fl = vh.hits(L, A, b, lb, ub, np.tile(st, (3, 1)), np.tile(inc, (3, 1)), 10, m=np.array([0, 4, 4], np.int32))
    assert list(fl) == [2, 1, 0]


# ---------------------------------------------------------------------------------------------- volume_batch, no device
def test_volume_batch_arguments():
    from polytope_amd import batch, _lib
    import polytope_amd
    assert polytope_amd.volume_batch is batch.volume_batch
    assert sorted(n for n in _lib.SIGNATURES if "volume" in n) == ["plp_volume_hits", "plp_volume_hits_dev"]
    A = np.zeros((3, 4, 2))
    b = np.ones((3, 4))
    box = dict(lb=-np.ones((3, 2)), ub=np.ones((3, 2)))
    with pytest.raises(ValueError, match="must be \\[B, m_max, d\\]"):
        batch.volume_batch(A[0], b[0])
    with pytest.raises(ValueError, match="`nsamples` must be >= 1"):
        batch.volume_batch(A, b, nsamples=0, **box)
    with pytest.raises(ValueError, match="`nsamples` must be >= 1"):
        batch.volume_batch(A, b, nsamples=-3, **box)
    with pytest.raises(ValueError, match="noninteger number of samples"):
        batch.volume_batch(A, b, nsamples=10.5, **box)
    with pytest.raises(ValueError, match="2\\^31 - 1"):
        batch.volume_batch(A, b, nsamples=2 ** 31, **box)
    with pytest.raises(ValueError, match="2 seeds for 3 polytopes"):
        batch.volume_batch(A, b, seed=[1, 2], **box)
    with pytest.raises(ValueError, match="non-negative"):
        batch.volume_batch(A, b, seed=-1, **box)
    with pytest.raises(TypeError):
        batch.volume_batch(A, b, seed=[1, 2.5, 3], **box)
    with pytest.raises(TypeError):
        batch.volume_batch(A, b, seed=np.random.default_rng(1), **box)
    with pytest.raises(ValueError, match="lb and ub come together"):
        batch.volume_batch(A, b, lb=box["lb"])
    with pytest.raises(ValueError, match="lb / ub must be"):
        batch.volume_batch(A, b, lb=np.zeros((3, 3)), ub=np.zeros((3, 3)))
    # the reference's table by dimension
    assert [batch._volume_nsamples(d) for d in (1, 2, 3, 4, 16)] == [50, 500, 3000, 10000, 10000]
    assert batch._volume_nsamples(2, 77) == 77


def test_volume_batch_seed_forms():
    """None: spawned children of one SeedSequence (distinct streams); an int: the same stream B times; B ints: one each.
    The words handed to the library are PCG64(seed)'s state and increment."""
    from polytope_amd import batch
    s = batch._volume_seeds(5, 3)
    assert s == [5, 5, 5]
    assert batch._volume_seeds([4, np.int64(5), 2 ** 100], 3) == [4, 5, 2 ** 100]
    kids = batch._volume_seeds(None, 4)
    assert len(kids) == 4 and all(isinstance(c, np.random.SeedSequence) for c in kids)
    st, inc = batch._pcg64_words(kids + [5, 5])
    assert st.shape == (6, 2) and st.dtype == np.uint64 and len({tuple(r) for r in st[:4]}) == 4
    for row_s, row_i, sd in zip(st, inc, kids + [5, 5]):
        want = np.random.PCG64(sd).state["state"]
        assert int(row_s[0]) | (int(row_s[1]) << 64) == want["state"]
        assert int(row_i[0]) | (int(row_i[1]) << 64) == want["inc"]


def test_volume_batch_without_a_device_raises():
    from polytope_amd import batch, _lib
    if _lib.available():
        pytest.skip("GPU present")
    A = np.zeros((1, 4, 2))
    A[0] = [[1, 0], [-1, 0], [0, 1], [0, -1]]
    with pytest.raises(_lib.PlpError):
        batch.volume_batch(A, np.ones((1, 4)), seed=1, lb=-np.ones((1, 2)), ub=np.ones((1, 2)))
    with pytest.raises(_lib.PlpError):
        batch.volume_batch(A, np.ones((1, 4)), seed=1)
