"""Host build of polytope_amd/csrc/plp_rdiff_search.hpp (tests/cabi/rdiff_search_host.cpp, g++ -ffp-contract=off) for
tests/test_rdiff_search_host.py: the library's region_diff search on the CPU, its radii from a Python function, so that
it can be held against polytope._DiffSearch piece for piece; and the random cases of the GPU parity test."""
import ctypes as C
import os

import numpy as np

import host_build as hb

SRC = os.path.join(hb.ROOT, "tests", "cabi", "rdiff_search_host.cpp")
OK, SCAN_MEMO, RADIUS_MISSING, BAD_INDEX, LIST_TOO_LONG = 0, -1, -2, -3, -4   # plp::rdiff::Err
DEFAULT_KNOBS = (100, 6, 8, 0, 1)   # sib, chain_scan, chain_node, deep, child
NO_SPECULATION = (0, 0, 0, 0, 0)
_CB = C.CFUNCTYPE(C.c_int, C.c_longlong, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_double), C.c_void_p)


def build(tmpdir):
    L = C.CDLL(hb.build(SRC, "librdiff_search_host.so", tmpdir))
    L.rdiff_search_host.restype = C.c_int
    L.rdiff_search_host.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_double, C.c_void_p, C.c_longlong, C.c_longlong,
                                    C.c_longlong, _CB, C.c_void_p, C.c_longlong, C.c_longlong, C.c_void_p, C.c_void_p,
                                    C.c_void_p, C.c_void_p]
    L.rdiff_move_host.restype = C.c_int
    L.rdiff_move_host.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_longlong, C.c_void_p, C.c_void_p, C.c_int,
                                  C.c_longlong, C.c_void_p, C.c_void_p, C.c_void_p]
    return L


def move(L, m, mi, counter, idx, level, which):
    """One move of plp::rdiff::State on a hand-made state (which: 0 = next_sibling, 1 = reopen_after_piece), then
    resolve -> (level, ended, counter, idx, sum of the counters, table rows or None where an index is out of range)."""
    mi = np.ascontiguousarray(mi, dtype=np.int32)
    cnt = np.array(counter, dtype=np.int32)
    src = np.array(idx, dtype=np.int64)
    lvl = np.array([level], dtype=np.int64)
    cap = len(idx) + 2
    idx_out, rows_out, out = np.zeros(cap, np.int64), np.zeros(cap, np.int32), np.zeros(4, np.int64)
    rc = L.rdiff_move_host(int(m), int(mi.size), hb.ptr(mi), hb.ptr(cnt), len(idx), hb.ptr(src), hb.ptr(lvl), int(which), cap,
                           hb.ptr(idx_out), hb.ptr(rows_out), hb.ptr(out))
    assert rc == 0
    n = int(out[2])
    return (int(lvl[0]), bool(out[0]), [int(v) for v in cnt], [int(v) for v in idx_out[:n]], int(out[3]),
            [int(v) for v in rows_out[:n]] if out[1] else None)


def build_program(tmpdir):
    """The stand-alone program (-DRDIFF_HOST_MAIN) under -fsanitize=address,undefined -> its path."""
    return hb.build_program(SRC, "RDIFF_HOST_MAIN", "rdiff_search_host_san", tmpdir)


class Outcome(object):
    """code: plp::rdiff::Err; leaves: [(kind, rows tuple)]; n_requests / n_scan_miss / n_node_miss; batches: the lists
    (row tuples) of every sub-batch handed to the backend, in order."""

    def __init__(self, code, leaves, counts, batches):
        self.code, self.leaves, self.batches = code, leaves, batches
        self.n_requests, self.n_scan_miss, self.n_node_miss = (int(v) for v in counts[2:5])

    @property
    def asked(self):
        return [w for b in self.batches for w in b]


def search(L, m, mi, abs_tol, radii_of, knobs=None, cap_lp=0, cap_rows=0, memo_limit=0):
    """Runs the host-built search.  radii_of(list of row tuples) -> radii (NaN = no verdict)."""
    mi = np.ascontiguousarray(mi, dtype=np.int32)
    batches, raised = [], []

    def cb(n, off, rows, out, _user):
        try:
            lists = [tuple(rows[off[k]:off[k + 1]]) for k in range(n)]
            batches.append(lists)
            for k, r in enumerate(radii_of(lists)):
                out[k] = r
            return 0
        except BaseException as e:   # (an exception cannot cross the C frames: end the search, raise it afterwards)
            raised.append(e)
            return 99
    kn = None if knobs is None else np.asarray(knobs, dtype=np.int32)
    max_leaves, max_rows = 1 << 12, 1 << 18
    while True:
        kind, off, rows = np.zeros(max_leaves, np.int32), np.zeros(max_leaves + 1, np.int32), np.zeros(max_rows, np.int32)
        counts = np.zeros(5, np.int64)
        del batches[:]
        code = L.rdiff_search_host(int(m), int(mi.size), hb.ptr(mi), float(abs_tol), hb.ptr(kn), cap_lp, cap_rows, memo_limit,
                                   _CB(cb), None, max_leaves, max_rows, hb.ptr(kind), hb.ptr(off), hb.ptr(rows), hb.ptr(counts))
        if raised:
            raise raised[0]
        if code != -100:
            break
        max_leaves, max_rows = int(counts[0]) + 1, int(counts[1]) + 1
    leaves = [(int(kind[k]), tuple(int(v) for v in rows[off[k]:off[k + 1]])) for k in range(int(counts[0]))]
    return Outcome(code, leaves, counts, batches)


def random_cases(n_trials):
    """The first `n_trials` (at most 24) polytope / cells pairs of test_region_diff_library_search_equals_host_loop
    (tests/test_gpu_parity.py): default_rng(77), d = 2, 3, 4 in turn, 3..13 overlapping boxes against a random polytope."""
    import polytope_amd.polytope as pcm
    rng = np.random.default_rng(77)
    out = []
    for trial in range(n_trials):
        d = 2 + trial % 3
        n = int(rng.integers(3, 14))
        cen = rng.random((n, d))
        hw = rng.uniform(0.05, 0.3, (n, d))
        cells = [pcm.box2poly(np.c_[c - w, c + w].tolist()) for c, w in zip(cen, hw)]
        A = rng.standard_normal((3 * d, d))
        A /= np.linalg.norm(A, axis=1)[:, None]
        out.append((pcm.Polytope(A, 0.3 * (1 + rng.random(3 * d)) + A @ (0.5 * np.ones(d))), cells))
    return out
