"""CPU: the two forms of walk3 (polytope_amd/csrc/plp_lane_lp.hpp) -- the plain general loop (-DPLP_LANE_PLAIN_WALK) and
the default one with its second and third pass peeled and the active rows fetched together -- compiled
for the host from the same header and run on every box (F3) and redundancy (F2) LP of the families of
tests/lane_walk_cases.py and the structured polytopes, d = 1, 2, 3 embedded in R^3.  The final Lp3 of every LP must be the
same field by field, doubles as bit patterns, and every exit of the walk must have been taken in each form."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

SRC = os.path.join(ROOT, "tests", "cabi", "lane_walk_ab_host.cpp")
FLAGS = ["-O2", "-std=c++17", "-ffp-contract=off", "-fPIC"]
# plp::lane::WE_* (plp_lane_lp.hpp)
TALLY = ["opt1", "opt2", "opt3", "unbnd", "retry_pair", "retry_triple", "retry_degen", "drop2", "drop3",
         "pass_facet", "pass_edge", "pass_general"]


@pytest.fixture(scope="module")
def built(tmp_path_factory):
    d = tmp_path_factory.mktemp("lane_walk_ab")
    plain, peeled, main = str(d / "plain.o"), str(d / "peeled.o"), str(d / "peeled_main.o")
    subprocess.check_call(["g++", *FLAGS, "-DPLP_LANE_PLAIN_WALK", "-c", SRC, "-o", plain])
    subprocess.check_call(["g++", *FLAGS, "-c", SRC, "-o", peeled])
    subprocess.check_call(["g++", *FLAGS, "-DLANE_WALK_AB_MAIN", "-c", SRC, "-o", main])
    so, exe = str(d / "liblane_walk_ab.so"), str(d / "lane_walk_ab")
    subprocess.check_call(["g++", "-shared", "-o", so, plain, peeled])
    subprocess.check_call(["g++", "-o", exe, plain, main])
    return so, exe


@pytest.fixture(scope="module")
def forms(built):
    L = C.CDLL(built[0])
    dp, ip, lp = C.POINTER(C.c_double), C.POINTER(C.c_int), C.POINTER(C.c_longlong)
    fns = {}
    for name in ("plain", "peeled"):
        f = getattr(L, "lane_walk_run_" + name)
        f.argtypes = [C.c_longlong, C.c_int, dp, dp, dp, ip, dp, ip, lp]
        f.restype = C.c_longlong
        fns[name] = f

    def run(name, dim, A, beta, relax, mrows, tally):
        f = fns[name]
        args = (A.shape[0], dim, A.ctypes.data_as(dp), beta.ctypes.data_as(dp), relax.ctypes.data_as(dp), mrows.ctypes.data_as(ip))
        n = f(*args, None, None, None)
        xs, is_ = np.zeros((n, 3)), np.zeros((n, 7), np.int32)
        assert f(*args, xs.ctypes.data_as(dp), is_.ctypes.data_as(ip), tally.ctypes.data_as(lp)) == n
        return xs, is_
    return run


def _centred(oracle, A, b, mrows):
    """the polytopes with a Chebyshev ball, as the kernel hands them to the walk: rows in R^3, beta = max(b - A xc, 0) and
    the relaxed right-hand sides max((b + 0.1) - A xc, 0) of the redundancy LPs (polytope.py:1149)"""
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


def test_both_forms_of_the_walk_end_every_lp_in_the_same_state(forms, oracle):
    from lane_walk_cases import families
    from structured_cases import structured_polytopes
    tally = {"plain": np.zeros(len(TALLY), np.int64), "peeled": np.zeros(len(TALLY), np.int64)}
    lps = 0
    batches = [(d, fam) for d in (1, 2, 3) for fam in families(700, d)]
    As, bs, _ = structured_polytopes(1024)
    batches.append((3, ("structured", As, bs, np.full(1024, 16, np.int32))))
    for d, (name, A, b, mrows) in batches:
        A3, beta, relax, mr = _centred(oracle, A, b, mrows)
        assert len(mr) >= 100, (d, name, len(mr))   # (polytopes without a bounded ball never reach the walk)
        xp, ip_ = forms("plain", d, A3, beta, relax, mr, tally["plain"])
        xq, iq = forms("peeled", d, A3, beta, relax, mr, tally["peeled"])
        lps += len(xp)
        assert np.array_equal(ip_, iq), (d, name, "w0 w1 w2 nact status iters ndeg")
        assert np.array_equal(xp.view(np.uint64), xq.view(np.uint64)), (d, name, "x0 x1 x2")
    assert lps > 100000
    for form in ("plain", "peeled"):
        t = dict(zip(TALLY, tally[form].tolist()))
        print(form, t)
        for exit_ in ("opt1", "opt2", "opt3", "unbnd", "retry_pair", "retry_triple", "retry_degen", "drop2", "drop3"):
            assert t[exit_] > 0, (form, exit_, t)
    # exits are properties of the LP, not of the form; the peeled form takes most passes outside the general loop
    assert np.array_equal(tally["plain"][:9], tally["peeled"][:9])
    p, q = dict(zip(TALLY, tally["plain"].tolist())), dict(zip(TALLY, tally["peeled"].tolist()))
    assert p["pass_facet"] == p["pass_edge"] == 0
    assert min(q["pass_facet"], q["pass_edge"]) > 0
    assert q["pass_facet"] + q["pass_edge"] + q["pass_general"] == p["pass_general"]


def test_stand_alone_program_of_both_forms(built):
    """the program sanitizer runs are made with (its own batches, centre at the origin): here without a sanitizer"""
    out = subprocess.run([built[1]], stdout=subprocess.PIPE, universal_newlines=True)
    assert out.returncode == 0 and "0 batches differ" in out.stdout, out.stdout
