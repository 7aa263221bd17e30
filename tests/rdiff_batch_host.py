"""Host build of polytope_amd/csrc/plp_rdiff_batch.hpp (tests/cabi/rdiff_batch_host.cpp, g++ -ffp-contract=off) for
tests/test_rdiff_batch_host.py: the sequential rule of rdiff_batch_kernel on the CPU -- table build, single moves and the
search, its radii from a Python function -- and what the CPU and GPU tests of region_diff_batch share: packing problems,
reading leaves, the table region_diff builds in numpy."""
import ctypes as C
import os

import numpy as np

import host_build as hb
import rdiff_host as RH

SRC = os.path.join(hb.ROOT, "tests", "cabi", "rdiff_batch_host.cpp")
RD_OK, RD_OVERFLOW, RD_COVERED, RD_LONG, RD_BUDGET, RD_INDEX, RD_UNSUPPORTED = range(7)   # plp::rdb::Status
MAX_LIST, MAX_TABLE, MAX_NEW = 64, 256, 127
_CB = RH._CB


def build(tmpdir):
    L = C.CDLL(hb.build(SRC, "librdiff_batch_host.so", tmpdir))
    vp, i, ll, dbl = C.c_void_p, C.c_int, C.c_longlong, C.c_double
    L.rdiff_batch_host.restype = i
    L.rdiff_batch_host.argtypes = [i, i, vp, vp, ll, i, vp, vp, vp, i, vp, dbl, i, i, i, _CB, vp, vp, vp, vp, vp, vp, vp, i, vp]
    L.rdiff_batch_search_host.restype = i
    L.rdiff_batch_search_host.argtypes = [i, i, vp, dbl, i, i, i, _CB, vp, vp, vp, vp, vp]
    L.rdiff_batch_move_host.restype = i
    L.rdiff_batch_move_host.argtypes = [i, i, vp, vp, ll, vp, vp, i, ll, vp, vp, vp]
    return L


def build_program(tmpdir):
    """The stand-alone program (-DRDIFF_BATCH_HOST_MAIN) under -fsanitize=address,undefined -> its path."""
    return hb.build_program(SRC, "RDIFF_BATCH_HOST_MAIN", "rdiff_batch_host_san", tmpdir)


class Outcome(object):
    """status / count / nrows / nlp as the kernel reports them; leaves: the [(kind, rows tuple)] that were written; asked:
    the lists (row tuples) whose radius the rule read, in order; mi, src, M, table (build only)."""

    def __init__(self, out, kind, off, rows, p_max, asked):
        self.count, self.nrows, self.nlp, self.status = (int(v) for v in out[:4])
        n = min(self.count, p_max)
        for k in range(n):   # (what fits is written: the pieces in front of the first that did not, whose off is -1)
            if off[k + 1] < 0:
                n = k
                break
        self.leaves = [(int(kind[k]), tuple(int(v) for v in rows[off[k]:off[k + 1]])) for k in range(n)]
        self.asked = asked


def _callback(radii_of, asked, raised):
    def cb(n, off, rows, out, _user):
        try:
            lists = [tuple(rows[off[k]:off[k + 1]]) for k in range(n)]
            asked.extend(lists)
            for k, r in enumerate(radii_of(lists)):
                out[k] = r
            return 0
        except BaseException as e:   # (an exception cannot cross the C frames: end the search, raise it afterwards)
            raised.append(e)
            return 99
    return _CB(cb)


def search(L, m, mi, abs_tol, radii_of, max_lps=1 << 16, p_max=1 << 12, r_max=1 << 18):
    """The search alone on the table shape (m, mi).  radii_of(list of row tuples) -> radii (NaN = no verdict)."""
    mi = np.ascontiguousarray(mi, dtype=np.int32)
    # (zeros: an overflowing search leaves the slots past what fits unwritten, and Outcome reads off[] to find them)
    kind, off, rows = np.zeros(p_max, np.int32), np.zeros(p_max + 1, np.int32), np.zeros(r_max, np.int32)
    out, asked, raised = np.zeros(5, np.int64), [], []
    rc = L.rdiff_batch_search_host(int(m), int(mi.size), hb.ptr(mi), float(abs_tol), int(max_lps), int(p_max), int(r_max),
                                   _callback(radii_of, asked, raised), None, hb.ptr(kind), hb.ptr(off), hb.ptr(rows), hb.ptr(out))
    if raised:
        raise raised[0]
    assert rc == 0
    return Outcome(out, kind, off, rows, p_max, asked)


def problem(L, A, b, CA, Cb, mc, cell_idx, abs_tol, radii_of, max_lps=1 << 16, p_max=1 << 12, r_max=1 << 18):
    """One problem through table build and search: minuend A[m, d], b[m]; the cells cell_idx of CA[Nc, mc_max, d], Cb, mc."""
    A, b = np.ascontiguousarray(A, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    CA, Cb = np.ascontiguousarray(CA, dtype=np.float64), np.ascontiguousarray(Cb, dtype=np.float64)
    mc, cell_idx = np.ascontiguousarray(mc, dtype=np.int32), np.ascontiguousarray(cell_idx, dtype=np.int32)
    m, d = A.shape
    Nc, mc_max = Cb.shape
    N = cell_idx.size
    kind, off, rows = np.zeros(p_max, np.int32), np.zeros(p_max + 1, np.int32), np.zeros(r_max, np.int32)
    out, asked, raised = np.zeros(5, np.int64), [], []
    mi, src, table = np.zeros(max(N, 1), np.int32), np.full(MAX_NEW, -1, np.int32), np.full((MAX_TABLE, d + 1), np.nan)
    rc = L.rdiff_batch_host(d, m, hb.ptr(A), hb.ptr(b), Nc, mc_max, hb.ptr(CA), hb.ptr(Cb), hb.ptr(mc), N, hb.ptr(cell_idx),
                            float(abs_tol), int(max_lps), int(p_max), int(r_max), _callback(radii_of, asked, raised), None,
                            hb.ptr(kind), hb.ptr(off), hb.ptr(rows), hb.ptr(out), hb.ptr(mi), hb.ptr(src), MAX_NEW, hb.ptr(table))
    if raised:
        raise raised[0]
    assert rc == 0
    o = Outcome(out, kind, off, rows, p_max, asked)
    o.M = int(out[4])
    o.mi, o.src = mi[:N].copy(), src[:o.M].copy()
    o.table = table[:m + 2 * o.M].copy() if o.status != RD_UNSUPPORTED else None
    return o


def move(L, m, mi, counter, idx, level, which):
    """One move of plp::rdb::State on a hand-made state: what rdiff_host.move returns for plp::rdiff::State."""
    mi = np.ascontiguousarray(mi, dtype=np.int32)
    cnt = np.array(counter, dtype=np.int32)
    src = np.array(idx, dtype=np.int64)
    lvl = np.array([level], dtype=np.int64)
    cap = len(idx) + 2
    idx_out, rows_out, out = np.zeros(cap, np.int64), np.zeros(cap, np.int32), np.zeros(4, np.int64)
    rc = L.rdiff_batch_move_host(int(m), int(mi.size), hb.ptr(mi), hb.ptr(cnt), len(idx), hb.ptr(src), hb.ptr(lvl), int(which),
                                 cap, hb.ptr(idx_out), hb.ptr(rows_out), hb.ptr(out))
    assert rc == 0, rc
    n = int(out[2])
    return (int(lvl[0]), bool(out[0]), [int(v) for v in cnt], [int(v) for v in idx_out[:n]], int(out[3]),
            [int(v) for v in rows_out[:n]] if out[1] else None)


def numpy_table(pA, pb, cells, abs_tol):
    """The table region_diff builds (polytope.py:1726-1741) for the minuend (pA, pb) and the ordered `cells` [(A, b)]:
    the same numpy expressions -> (A[m + 2M, d], B[m + 2M], mi[N]) (region_diff itself stops before the negations when
    an mi is 0)."""
    m = pA.shape[0]
    base = np.hstack([pA, pb[:, None]])
    rows_all = np.vstack([np.hstack([cA, cb[:, None]]) for cA, cb in cells])
    owner = np.concatenate([np.full(cA.shape[0], ii) for ii, (cA, _) in enumerate(cells)])
    new = np.all(np.sum(np.abs(rows_all[:, None, :] - base[None, :, :]), axis=2) >= abs_tol, axis=1)
    mi = np.bincount(owner[new], minlength=len(cells)).astype(int)
    A = np.vstack([pA, rows_all[new, :-1]])
    B = np.hstack([pb, rows_all[new, -1]])
    M = int(np.sum(mi))
    return np.vstack([A, -A[m:m + M, :]]), np.hstack([B, -B[m:m + M]]), mi


def pack_cells(cells):
    """[(A, b)] -> CA[Nc, mc_max, d], Cb[Nc, mc_max], mc[Nc] (zero padding)."""
    mc = np.array([c[0].shape[0] for c in cells], dtype=np.int32)
    d = cells[0][0].shape[1]
    CA, Cb = np.zeros((len(cells), int(mc.max()), d)), np.zeros((len(cells), int(mc.max())))
    for k, (cA, cb) in enumerate(cells):
        CA[k, :mc[k]], Cb[k, :mc[k]] = cA, cb
    return CA, Cb, mc
