"""CPU: is_convex_batch / envelope_batch on the default backend against the reference's verdicts and envelopes of whole
regions (tests/golden/g25_convex_regions.npz: hyperplane splits, splits with a piece removed, overlapping, separated,
nested and duplicated members, d = 2..4, 2..8 members).  On this backend both calls are the loop of single calls: what is
checked is the public surface and, through it, envelope / is_convex on regions of more than two members."""
import numpy as np
import pytest

from conftest import load_golden


@pytest.fixture(scope="module")
def g25():
    return load_golden("g25_convex_regions.npz")


def _regions(g, pcm, ks):
    out = []
    for k in ks:
        d = int(g["d"][k])
        out.append(pcm.Region([pcm.Polytope(g["A"][k, q, :g["m"][k, q], :d].copy(), g["b"][k, q, :g["m"][k, q]].copy(),
                                            normalize=False) for q in range(int(g["n"][k]))]))
    return out


def _check_rows(g, k, env):
    """The envelope's rows against the fixture's, to the tolerance test_python_api.py holds g11 / g21 to."""
    d, m = int(g["d"][k]), int(g["env_m"][k])
    assert env.A.shape[0] == m, (k, env.A.shape[0], m)
    if m:
        ref = g["env_Ab"][k, :m]
        assert np.allclose(np.c_[env.A, env.b], np.c_[ref[:, :d], ref[:, 4]], rtol=0, atol=1e-9), k


def test_fixture_is_what_the_generator_promises(g25):
    g = g25
    N = len(g["d"])
    assert N >= 48 and set(g["d"].tolist()) == {2, 3, 4} and g["n"].min() == 2 and g["n"].max() == 8
    assert set(g["kind"].tolist()) == set(range(len(g["kinds"])))
    assert 0 < g["convex"].sum() < N
    # rows are unit length, as the constructor leaves them
    live = np.arange(g["A"].shape[2])[None, None, :] < g["m"][:, :, None]
    assert np.allclose(np.sqrt(np.sum(g["A"] ** 2, 3))[live], 1.0, rtol=0, atol=1e-12)


@pytest.mark.parametrize("part", range(3))
def test_batch_calls_give_the_references_answers(g25, part):
    """is_convex_batch: the reference's bool for every region, and its envelope where the region is convex; envelope_batch:
    the reference's envelope rows, convex or not (an empty polytope where the reference returns one)."""
    import polytope_amd
    import polytope_amd.polytope as pcm
    g = g25
    ks = [k for k in range(len(g["d"])) if int(g["d"][k]) == 2 + part]
    got = polytope_amd.is_convex_batch(_regions(g, pcm, ks))
    assert len(got) == len(ks)
    for k, (conv, outer) in zip(ks, got):
        assert bool(conv) == bool(g["convex"][k]), k
        assert (outer is not None) == bool(conv), k
        if conv:
            _check_rows(g, k, outer)
    # (the envelope of a convex region was checked above; on this backend a second pass would only repeat its LP loop)
    rest = [k for k in ks if not g["convex"][k]]
    env = polytope_amd.envelope_batch(_regions(g, pcm, rest))
    assert len(env) == len(rest)
    for k, e in zip(rest, env):
        _check_rows(g, k, e)


def test_lengths_empty_regions_and_what_the_single_call_raises():
    import polytope_amd
    import polytope_amd.polytope as pcm
    box = pcm.box2poly([[0.0, 1.0], [0.0, 1.0]])
    assert polytope_amd.is_convex_batch([]) == [] and polytope_amd.envelope_batch([]) == []
    got = polytope_amd.is_convex_batch([pcm.Region(), box, pcm.Region([box, pcm.box2poly([[1.0, 2.0], [0.0, 1.0]])])])
    assert got[0] == (True, None) and got[1] == (True, None) and bool(got[2][0]) and got[2][1].A.shape == (4, 2)
    with pytest.raises(AttributeError):
        polytope_amd.envelope_batch([pcm.Region()])
    # abs_tol <= 0 goes through the single calls as well
    one = pcm.Region([box.copy(), pcm.box2poly([[1.0, 2.0], [0.0, 1.0]])])
    want = pcm.envelope(one, abs_tol=0.0)
    got = polytope_amd.envelope_batch([pcm.Region([p.copy() for p in one.list_poly])], abs_tol=0.0)[0]
    assert np.array_equal(got.A, want.A) and np.array_equal(got.b, want.b)
