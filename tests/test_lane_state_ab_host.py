"""CPU: walk3 (polytope_amd/csrc/plp_lane_lp.hpp) with the vertex round in its general loop (the default) and without
(-DPLP_LANE_WIDE_STATE -DPLP_LANE_NO_VERTEX_ROUND; the walk's integer state has one form, the fields of Lp3, so the first
flag changes nothing), compiled for the host from the same header and run on every box (F3) and redundancy (F2) LP of the
families of tests/lane_walk_cases.py, d = 1, 2, 3 embedded in R^3, from the centre and (the box LPs) warm from a vertex,
an edge and a facet point.  The final Lp3 of every LP must be the same field by field, doubles as bit patterns -- the -1
of a slot never filled and the stale row a slot keeps after a drop included -- and so must every tally of the walk but
the two pass kinds the vertex round moves passes between."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

SRC = os.path.join(ROOT, "tests", "cabi", "lane_state_ab_host.cpp")
FLAGS = ["-O2", "-std=c++17", "-ffp-contract=off", "-fPIC"]
WIDE = ["-DPLP_LANE_WIDE_STATE", "-DPLP_LANE_NO_VERTEX_ROUND"]
# plp::lane::WE_* (plp_lane_lp.hpp)
TALLY = ["opt1", "opt2", "opt3", "unbnd", "retry_pair", "retry_triple", "retry_degen", "drop2", "drop3",
         "pass_facet", "pass_edge", "pass_general", "pass_vertex"]


@pytest.fixture(scope="module")
def built(tmp_path_factory):
    d = tmp_path_factory.mktemp("lane_state_ab")
    wide, packed, main = str(d / "wide.o"), str(d / "packed.o"), str(d / "packed_main.o")
    subprocess.check_call(["g++", *FLAGS, *WIDE, "-c", SRC, "-o", wide])
    subprocess.check_call(["g++", *FLAGS, "-c", SRC, "-o", packed])
    subprocess.check_call(["g++", *FLAGS, "-DLANE_STATE_AB_MAIN", "-c", SRC, "-o", main])
    so, exe = str(d / "liblane_state_ab.so"), str(d / "lane_state_ab")
    subprocess.check_call(["g++", "-shared", "-o", so, wide, packed])
    subprocess.check_call(["g++", "-o", exe, wide, main])
    return so, exe


@pytest.fixture(scope="module")
def forms(built):
    L = C.CDLL(built[0])
    dp, ip, lp = C.POINTER(C.c_double), C.POINTER(C.c_int), C.POINTER(C.c_longlong)
    fns = {}
    for name in ("wide", "packed"):
        f = getattr(L, "lane_state_run_" + name)
        f.argtypes = [C.c_longlong, C.c_int, dp, dp, dp, ip, dp, ip, lp, lp]
        f.restype = C.c_longlong
        fns[name] = f

    def run(name, dim, A, beta, relax, mrows, tally, warm_from):
        cap = A.shape[0] * (4 * dim + 16)   # 2 dim box LPs, at most 16 redundancy LPs, 2 dim warm starts per polytope
        xs, is_ = np.zeros((cap, 3)), np.zeros((cap, 7), np.int32)
        n = fns[name](A.shape[0], dim, A.ctypes.data_as(dp), beta.ctypes.data_as(dp), relax.ctypes.data_as(dp),
                      mrows.ctypes.data_as(ip), xs.ctypes.data_as(dp), is_.ctypes.data_as(ip), tally.ctypes.data_as(lp),
                      warm_from.ctypes.data_as(lp))
        assert 0 < n <= cap
        return xs[:n], is_[:n]
    return run


def _centred(oracle, A, b, mrows):
    """the polytopes with a Chebyshev ball, as the kernel hands them to the walk (tests/test_lane_walk_ab_host.py)"""
    B, m, d = A.shape
    A3, beta, relax, mr = [], [], [], []
    for k in range(B):
        mk = int(mrows[k])
        st, r, xc = oracle.cheby(A[k, :mk], b[k, :mk])
        if st != 0 or not r > 1e-7:
            continue
        a = np.zeros((16, 3))
        a[:mk, :d] = A[k, :mk]
        s = A[k, :mk] @ np.asarray(xc).ravel()[:d]
        bt, rl = np.zeros(16), np.zeros(16)
        bt[:mk] = np.maximum(b[k, :mk] - s, 0.0)
        rl[:mk] = np.maximum((b[k, :mk] + 0.1) - s, 0.0)
        A3.append(a); beta.append(bt); relax.append(rl); mr.append(mk)
    return (np.ascontiguousarray(A3), np.ascontiguousarray(beta), np.ascontiguousarray(relax), np.asarray(mr, np.int32))


def test_with_and_without_the_vertex_round_every_lp_ends_in_the_same_state(forms, oracle):
    from lane_walk_cases import families
    tally = {f: np.zeros(len(TALLY), np.int64) for f in ("wide", "packed")}
    warm = {f: np.zeros(4, np.int64) for f in ("wide", "packed")}
    lps = 0
    stale = 0
    for d, (name, A, b, mrows) in [(d, fam) for d in (1, 2, 3) for fam in families(700, d)]:
        A3, beta, relax, mr = _centred(oracle, A, b, mrows)
        assert len(mr) >= 100, (d, name, len(mr))   # (polytopes without a bounded ball never reach the walk)
        xp, ip_ = forms("wide", d, A3, beta, relax, mr, tally["wide"], warm["wide"])
        xq, iq = forms("packed", d, A3, beta, relax, mr, tally["packed"], warm["packed"])
        lps += len(xp)
        assert ip_.shape == iq.shape, (d, name)
        for col, field in enumerate(("w0", "w1", "w2", "nact", "status", "iters", "ndeg")):
            assert np.array_equal(ip_[:, col].view(np.uint32), iq[:, col].view(np.uint32)), (d, name, field)
        assert np.array_equal(xp.view(np.uint64), xq.view(np.uint64)), (d, name, "x0 x1 x2")
        # slots beyond nact: never filled (-1) or left behind by a drop (a row number) -- both kinds must be in the run
        beyond = np.arange(3)[None, :] >= iq[:, 3:4]
        stale += int(np.sum(beyond & (iq[:, :3] >= 0)))
        assert np.any(beyond & (iq[:, :3] == -1)), (d, name)
    assert lps > 100000 and stale > 0, (lps, stale)
    p, q = (dict(zip(TALLY, tally[f].tolist())) for f in ("wide", "packed"))
    print("wide", p, "\npacked", q, "\nwarm starts by nact", warm["packed"].tolist())
    # exits and drops are properties of the LP, not of the form; so are the peeled passes
    same = [t for t in TALLY if t not in ("pass_general", "pass_vertex")]
    for t in same:
        assert p[t] == q[t], (t, p, q)
    for exit_ in ("opt1", "opt2", "opt3", "unbnd", "retry_pair", "retry_triple", "drop2", "drop3"):
        assert q[exit_] > 0, (exit_, q)
    assert np.array_equal(warm["wide"], warm["packed"]) and np.all(warm["packed"][1:] > 0), warm   # facet, edge, vertex
    assert q["pass_vertex"] > 0 and p["pass_vertex"] == 0
    assert q["pass_general"] + q["pass_vertex"] == p["pass_general"]


def test_stand_alone_program_of_both_states(built):
    """the program sanitizer runs are made with (its own batches, centre at the origin): here without a sanitizer"""
    out = subprocess.run([built[1]], stdout=subprocess.PIPE, universal_newlines=True)
    assert out.returncode == 0 and "0 batches differ" in out.stdout, out.stdout
