"""Host build of polytope_amd/csrc/plp_envelope.hpp (tests/cabi/envelope_host.cpp, g++ -ffp-contract=off) for
tests/test_envelope_host.py: the rule of envelope_cross_kernel on the CPU, its radii from a Python function -- and what the
CPU and GPU tests of envelope_batch share: random regions, packing, the brute force that runs every test."""
import ctypes as C
import os

import numpy as np

import host_build as hb

SRC = os.path.join(hb.ROOT, "tests", "cabi", "envelope_host.cpp")
ENV_OK, ENV_OPEN, ENV_UNSUPPORTED = range(3)   # plp::env::Status
MAX_DIM, MAX_ROWS = 8, 63
_CB = C.CFUNCTYPE(C.c_int, C.c_longlong, C.c_longlong, C.c_int, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double),
                  C.c_void_p)


def build(tmpdir):
    L = C.CDLL(hb.build(SRC, "libenvelope_host.so", tmpdir))
    vp, i, ll, dbl = C.c_void_p, C.c_int, C.c_longlong, C.c_double
    L.envelope_host.restype = i
    L.envelope_host.argtypes = [i, ll, i, vp, vp, vp, ll, vp, ll, vp, dbl, _CB, vp, vp, vp, vp]
    return L


def build_program(tmpdir):
    """The stand-alone program (-DENVELOPE_HOST_MAIN) under -fsanitize=address,undefined -> its path."""
    return hb.build_program(SRC, "ENVELOPE_HOST_MAIN", "envelope_host_san", tmpdir)


class Outcome(object):
    """outer uint64[L], status[L], nlp[L]; asked: [(w, j, ii, stack array [n, d + 1])] in the order the rule asked."""

    def __init__(self, outer, status, nlp, asked):
        self.outer, self.status, self.nlp, self.asked = outer, status, nlp, asked


def run(L, A, b, mc, reg_off, mem_idx, abs_tol, radius_of):
    """The rule on the packed table A[C, mc_max, d], b, mc and the lists reg_off / mem_idx (None: the identity).
    radius_of(w, j, ii, stack) -> the radius of that test (NaN = no verdict)."""
    A, b = np.ascontiguousarray(A, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    mc = None if mc is None else np.ascontiguousarray(mc, dtype=np.int32)
    reg_off = np.ascontiguousarray(reg_off, dtype=np.int32)
    mem_idx = None if mem_idx is None else np.ascontiguousarray(mem_idx, dtype=np.int32)
    Cn, mc_max, d = A.shape
    B = reg_off.size - 1
    n = int(mem_idx.size if mem_idx is not None else reg_off[B])
    outer, status, nlp = np.full(n, 7, np.uint64), np.full(n, -1, np.int32), np.full(n, -1, np.int32)
    asked, raised = [], []

    def cb(w, j, ii, rows, stack, out, _user):
        try:
            st = np.ctypeslib.as_array(stack, shape=(rows, d + 1)).copy()
            asked.append((int(w), int(j), int(ii), st))
            out[0] = radius_of(int(w), int(j), int(ii), st)
            return 0
        except BaseException as e:   # (an exception cannot cross the C frames: end the call, raise it afterwards)
            raised.append(e)
            return 99
    rc = L.envelope_host(d, Cn, mc_max, hb.ptr(A), hb.ptr(b), hb.ptr(mc), B, hb.ptr(reg_off), n, hb.ptr(mem_idx), float(abs_tol),
                         _CB(cb), None, hb.ptr(outer), hb.ptr(status), hb.ptr(nlp))
    if raised:
        raise raised[0]
    assert rc == 0, rc
    return Outcome(outer, status, nlp, asked)


def member_of(reg_off, mem_idx, w):
    return int(w if mem_idx is None else mem_idx[w])


def stack_of(A, b, mc, c, own, ii):
    """[rows of member c; -row ii of member own] as an [mc[c] + 1, d + 1] array."""
    top = np.hstack([A[c, :mc[c]], b[c, :mc[c], None]])
    return np.vstack([top, -np.hstack([A[own, ii], b[own, ii]])[None, :]])


def brute_force(A, b, mc, reg_off, mem_idx, abs_tol, radius_of):
    """Every (i, ii, j) test of the reference's loops (ii outer, j inner), none skipped -> (outer uint64[L], open bool[L],
    nlp[L], radii: {(w, j, ii): R}).  A test without a verdict (NaN, or abs_tol / 2 < R < 2 abs_tol) neither crosses nor
    clears; `open`: some row is not crossed and has such a test."""
    B = len(reg_off) - 1
    n = int(len(mem_idx) if mem_idx is not None else reg_off[B])
    outer, opened, nlp, radii = np.zeros(n, np.uint64), np.zeros(n, bool), np.zeros(n, np.int64), {}
    for p in range(B):
        lo, hi = int(reg_off[p]), int(reg_off[p + 1])
        for w in range(lo, hi):
            own = member_of(reg_off, mem_idx, w)
            word = 0
            for ii in range(int(mc[own])):
                crossed = unclear = False
                for j in range(hi - lo):
                    if lo + j == w:
                        continue
                    c = member_of(reg_off, mem_idx, lo + j)
                    R = radius_of(w, j, ii, stack_of(A, b, mc, c, own, ii))
                    radii[(w, j, ii)] = R
                    nlp[w] += 1
                    if R != R or 0.5 * abs_tol < R < 2 * abs_tol:
                        unclear = True
                    elif R > abs_tol:
                        crossed = True
                if not crossed:
                    word |= 1 << ii
                    opened[w] = opened[w] or unclear
            outer[w] = np.uint64(word)
    return outer, opened, nlp, radii


def pack(members):
    """[(A, b)] -> A[C, mc_max, d], b[C, mc_max], mc[C] (zero padding)."""
    mc = np.array([a.shape[0] for a, _ in members], dtype=np.int32)
    d = members[0][0].shape[1]
    A, b = np.zeros((len(members), int(mc.max()), d)), np.zeros((len(members), int(mc.max())))
    for k, (a, bb) in enumerate(members):
        A[k, :mc[k]], b[k, :mc[k]] = a, bb
    return A, b, mc


def random_member(rng, d, m, centre, size):
    """m unit rows around `centre`: the first d + 1 are a simplex of inradius about `size` (bounded from d + 1 rows on;
    with fewer the member is unbounded), the rest random cuts."""
    rows = [-np.eye(d), np.ones((1, d)) / np.sqrt(d)]
    extra = rng.standard_normal((max(m - d - 1, 0), d))
    a = np.vstack(rows + [extra / np.linalg.norm(extra, axis=1, keepdims=True)])[:m] if m >= 1 else np.zeros((0, d))
    off = size * rng.uniform(0.6, 1.0, a.shape[0])
    return a, a @ centre + off


def random_region(rng, d, n_members, rows_lo, rows_hi):
    """n_members members of rows_lo .. rows_hi rows each, centres a fraction of their size apart (they overlap, touch or
    lie apart) -> [(A, b)]."""
    out = []
    for _ in range(n_members):
        m = int(rng.integers(rows_lo, rows_hi + 1))
        out.append(random_member(rng, d, m, rng.uniform(-1.0, 1.0, d), float(rng.uniform(0.4, 1.2))))
    return out


def lists_of(regions):
    """[[(A, b)]] -> (A, b, mc, reg_off): every member of every region once, in order (the identity list)."""
    flat = [mem for reg in regions for mem in reg]
    A, b, mc = pack(flat)
    reg_off = np.concatenate([[0], np.cumsum([len(reg) for reg in regions])]).astype(np.int32)
    return A, b, mc, reg_off
