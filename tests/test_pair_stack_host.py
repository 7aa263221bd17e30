"""CPU: the stack rule of plp_pair_stacks / plp_intersect_pairs (polytope_amd/csrc/plp_pair_stack.hpp, compiled for the host
by tests/pair_stack_host.py) against numpy's statement of the Polytope constructor on the stacked rows, bit for bit --
every d = 1..16 (both summation orders of the norm and the left-over loop at d = 9..15), ragged tables, dropped rows,
both orders of every pair; and the same cases through the stand-alone program under the sanitizers."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import pair_stack_host as H  # noqa: E402


@pytest.fixture(scope="module")
def L(tmp_path_factory):
    return H.build(tmp_path_factory.mktemp("pair_stack_host"))


@pytest.mark.parametrize("m_max", H.M_MAXES)
@pytest.mark.parametrize("d", H.DIMS)
def test_stacks_equal_numpy(L, d, m_max):
    A, b, m = H.table(d, m_max)
    pairs = H.all_pairs()
    rc, A_s, b_s, m_s = H.stacks(L, A, b, m, pairs)
    assert rc == 0
    wA, wb, wm = H.numpy_stacks(A, b, m, pairs)
    assert np.array_equal(m_s, wm)
    assert np.array_equal(A_s, wA) and np.array_equal(b_s, wb)   # (no NaN reached an output: array_equal would fail)
    # the dropped rows are dropped: cell 0 lost its tiny row, cell 2 its zero row
    t = int(np.nonzero((pairs[:, 0] == 0) & (pairs[:, 1] == 2))[0][0])
    assert m_s[t] == m[0] + m[2] - 2
    # (i, j) and (j, i) hold the same rows in the other order
    u = int(np.nonzero((pairs[:, 0] == 2) & (pairs[:, 1] == 0))[0][0])
    k2 = m[2] - 1
    assert np.array_equal(A_s[t, :m[0] - 1], A_s[u, k2:k2 + m[0] - 1]) and np.array_equal(A_s[t, m[0] - 1:m_s[t]], A_s[u, :k2])


@pytest.mark.parametrize("d,m_max", [(1, 4), (3, 16), (8, 32), (13, 4)])
def test_rows_beyond_m_are_not_read(L, d, m_max):
    A, b, m = H.table(d, m_max, pad=np.nan)
    A0, b0, _ = H.table(d, m_max, pad=0.0)
    pairs = H.all_pairs()
    got, want = H.stacks(L, A, b, m, pairs), H.stacks(L, A0, b0, m, pairs)
    assert got[0] == want[0] == 0
    for g, w in zip(got[1:], want[1:]):
        assert np.array_equal(g, w)


@pytest.mark.parametrize("d,m_max", [(2, 4), (9, 16)])
def test_full_table_without_m(L, d, m_max):
    A, b, _ = H.table(d, m_max, pad=0.0)
    rng = np.random.default_rng(5)
    A, b = rng.standard_normal(A.shape) * 3.0, rng.standard_normal(b.shape)
    pairs = H.all_pairs()
    rc, A_s, b_s, m_s = H.stacks(L, A, b, None, pairs)
    wA, wb, wm = H.numpy_stacks(A, b, None, pairs)
    assert rc == 0 and np.all(m_s == 2 * m_max)
    assert np.array_equal(A_s, wA) and np.array_equal(b_s, wb) and np.array_equal(m_s, wm)


def test_bad_pairs_rejected(L):
    A, b, m = H.table(3, 4)
    for bad in H.BAD_PAIRS:
        pairs = np.array([(0, 1), bad, (2, 3)], dtype=np.int32)
        assert L.psh_first_bad(7, 3, pairs.ctypes.data) == 1
        rc, A_s, b_s, m_s = H.stacks(L, A, b, m, pairs)
        assert rc == 1
        assert np.all(A_s == -7.0) and np.all(b_s == -7.0) and np.all(m_s == -7)   # nothing written
        # the unchecked form (what the device does): the bad pair is an empty stack, its neighbours are untouched by it
        rc, A_s, b_s, m_s = H.stacks(L, A, b, m, pairs, checked=False)
        good = H.stacks(L, A, b, m, pairs[[0, 2]])
        assert rc == 0 and m_s[1] == 0 and np.all(A_s[1] == 0.0) and np.all(b_s[1] == 0.0)
        assert np.array_equal(A_s[[0, 2]], good[1]) and np.array_equal(b_s[[0, 2]], good[2]) and np.array_equal(m_s[[0, 2]], good[3])
    assert L.psh_first_bad(7, len(H.all_pairs()), H.all_pairs().ctypes.data) == -1


def test_unsupported_sizes(L):
    A, b, m = H.table(3, 4)
    pairs = H.all_pairs()
    big = np.zeros((7, 33, 3))
    assert H.stacks(L, big, np.zeros((7, 33)), None, pairs)[0] == 2          # W = 66 > 64
    assert H.stacks(L, np.zeros((7, 4, 17)), np.zeros((7, 4)), None, pairs)[0] == 2   # d = 17


def test_empty_list(L):
    A, b, m = H.table(3, 4)
    rc, A_s, b_s, m_s = H.stacks(L, A, b, m, np.zeros((0, 2), np.int32))
    assert rc == 0 and A_s.shape == (0, 8, 3) and m_s.shape == (0,)


def test_standalone_program_under_sanitizers(L, tmp_path):
    """The same cases through the stand-alone program built with -fsanitize=address,undefined: it forms the stacks again in
    allocations of exactly each array's size and compares them with the ones recorded here."""
    exe = H.build_program(tmp_path)
    cases = []
    for d in H.DIMS:
        for m_max in H.M_MAXES:
            A, b, m = H.table(d, m_max, pad=np.nan)
            pairs = H.all_pairs()
            rc, A_s, b_s, m_s = H.stacks(L, A, b, m, pairs)
            assert rc == 0
            cases.append((A, b, m, pairs, A_s, b_s, m_s))
    path = os.path.join(str(tmp_path), "cases.bin")
    H.write_cases(path, cases)
    out = subprocess.run([exe, path], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert out.returncode == 0, out.stdout
    assert "%d cases" % len(cases) in out.stdout and "all equal" in out.stdout
