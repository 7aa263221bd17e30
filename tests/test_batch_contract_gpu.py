"""GPU: the packed-table contract of include/plp.h on the device, entry point by entry point and engine by engine --
rows from m[p] on, points from n[p] on, rows or points whose keep bit is clear and rows of Q beyond mq[p] do not exist, and
member p's answer depends on member p only.  (tests/test_batch_contract_host.py holds the rule headers to the same on the
CPU; the staging loops of the .hip files are device-only code and are held here.)

a. padding is not read, at the C ABI (the `_dev` forms with CUDA tensors under NaN, 1e300 and answer-changing finite
   padding; the host-pointer forms, which refuse inf / nan by design, under the finite one): every output bit for bit the
   zero-padded call's, which is itself made twice (every entry point is expected to be bit-reproducible).
b. the same at the Python calls that reduce over whole arrays on the way (extreme_batch(reduce=True, v_max=None),
   volume_batch without boxes, support_batch(xc=None, resolve=True), subset_batch beyond mq, projection_batch over two
   steps, hull_batch(f_max=None)).
c. members do not see each other: the batch reversed and rolled by 3 gives the same bits, permuted; member p alone (B = 1)
   gives what it gives inside B = 257 -- bit for bit where the kernel does not depend on B, verdicts equal and floats to the
   tolerance of test_reduce_lane_gpu._same for lpsolve / cheby / bbox / reduce, whose engine does.
d. an outside reference on the live rows only: the oracle for the LP family, contains and the pair kernels, the oracle's
   simplex for support, exact rational arithmetic for the vertices and facets of the lattice cases.

Kernels covered (the plans of tests/cabi/reduce_plan_host.cpp and tests/cabi/lp_plan_host.cpp are asked which engines the
cases below reach; test_engine_coverage and test_lp_engine_coverage assert it against REQUIRED / LP_REQUIRED):
  plp_reduce_batch       GENERAL (reduce_kernel), LANE at 16 / 8 / 4 lanes per polytope and 16 / 32 row slots
                         (reduce_lane_kernel), LANE_MIX (reduce_lane_mix_kernel, its default thresholds: 16 001 and 40 001
                         members), GROUP at 4 x 4 and 8 x 2 (reduce_r_kernel), GROUP_MIX half tiles and full + half tiles
                         (reduce_r_mix_kernel, 70 000 members), SPLIT (reduce_split_kernel), WDENSE, LAZY, WSPLIT at 2 and 4
                         wavefronts, with and without a stored dictionary
  plp_reduce_wide_batch  reduce_lds_kernel (70 rows), one member per workgroup and members in turn (33 025 members)
  plp_lp_solve_batch     GROUP with the phase-1 kernel and the retry pass (lp_r_kernel + lp_p1_r_kernel + lp_kernel), without
                         phase 1 at four and at two rows per lane, GENERAL alone (lp_kernel), WIDE (lp_w_kernel), LDS
                         (lp_lds_kernel) beyond 64 rows and with members in turn (PLP_LDS, 33 025 members)
  plp_cheby_batch        GROUP at four and two rows per lane (cheby_r_kernel), GENERAL (cheby_kernel), WIDE (cheby_w_kernel),
                         LDS (cheby_lds_kernel) likewise
  plp_bbox_batch         LANE (bbox_lane_kernel), SPLIT (bbox_split_kernel), GROUP (bbox_r_kernel), WIDE on four wavefronts
                         and on one (bbox_wsplit_kernel, bbox_lazy_kernel), each with and without a stored dictionary
  plp_contains           both modes
  plp_adjacent_pairs, plp_adjacent_pairs_range, plp_overlap_pairs, plp_overlap_cross
                         GROUP (adjacent_r_kernel) at 4, 8 and 16 lanes per pair, WIDE (adjacent_w_kernel); empty (by two
                         rows, by a zero row), flat and unbounded cells among the bounded ones, up to 257 cells
  plp_fm_count / plp_fm_emit   with m alone and with keep / flags of a reduce, first on and off, col < 0; one member per
                         workgroup and members in turn (33 025 members)
  plp_volume_hits        one tile per workgroup and the grid-stride loop (PLP_VOLUME_MAX_GRID)
  plp_support_batch      16 / 32 / 64 row slots, C shared and per polytope, K = 1 / 5 / 33 (64, 16, 8 and 1 polytopes per
                         workgroup)
  plp_extreme_batch, plp_hull_batch   d = 2, 3, 4, one round and many, keep words with holes
Every output of a raw call is filled with a byte pattern first, so that "every output bit" covers the slots a kernel leaves
unwritten.  m[p] is never outside 0 .. m_max: the header does not define that."""
import contextlib
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from polytope_amd import batch, solvers  # noqa: E402
import contract_cases as cc  # noqa: E402
import extreme_host as xh  # noqa: E402
import hull_host as hh  # noqa: E402
import support_host as sh  # noqa: E402
from test_reduce_plan import ENGINES, FIELDS, plan as reduce_plan  # noqa: E402,F401 (a fixture: the compiled plan)
from test_lp_plan import ENGINES as LP_ENGINES, plan as lp_plan  # noqa: E402,F401 (likewise, for the LP family)

pytestmark = pytest.mark.gpu

SIZES = (1, 5, 257)
TOL = 1e-9


# ------------------------------------------------------------------------------------------------ plumbing
@contextlib.contextmanager
def switches(env):
    """The A/B switches of one case in the environment (the library reads them per call), taken out again after."""
    env = {k: str(v) for k, v in (env or {}).items()}
    saved = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        yield
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def to_dev(v):
    import torch
    if not isinstance(v, np.ndarray):
        return v
    if v.dtype == np.uint64:
        v = v.view(np.int64)
    return torch.as_tensor(np.ascontiguousarray(v)).to("cuda:0")


def to_host(res):
    import torch
    if any(hasattr(v, "is_cuda") for v in res.values()):
        torch.cuda.synchronize()
    return {k: (v.cpu().numpy() if hasattr(v, "cpu") else np.asarray(v)) for k, v in res.items() if v is not None}


def run(fn, args, device):
    return to_host(fn(**({k: to_dev(v) for k, v in args.items()} if device else args)))


def assert_same(got, want, what, keys=None):
    for k in (keys or sorted(want)):
        assert cc.same_bits(got[k], want[k]), (what, k, np.argwhere(np.asarray(got[k]) != np.asarray(want[k]))[:4].tolist())


def assert_close(got, want, what):
    """The rule of tests/test_reduce_lane_gpu.py: _same -- integer fields (statuses, verdicts, counts) exact, radii and
    optimal values to 1e-12, points to 1e-9, NaN where NaN; pivot counts are not compared."""
    for k in sorted(want):
        if k == "iters":
            continue
        g, w = np.asarray(got[k]), np.asarray(want[k])
        if w.dtype.kind in "iub":
            assert np.array_equal(g, w), (what, k, np.argwhere(g != w)[:4].tolist())
        else:
            atol = 1e-12 if k in ("r", "fun") else 1e-9
            assert np.allclose(g, w, rtol=0.0, atol=atol, equal_nan=True), (what, k, float(np.nanmax(np.abs(g - w))))


class Case:
    """One entry point on one batch: fn(**args) -> dict of outputs.  `tables`: what has padding, as tuples
    (names of the arrays, name of the count, name of the keep word or None, "rows" / "points"); `members`: the arguments
    with one entry per member (they are permuted and sliced with the batch; every output follows along its first axis);
    `bitwise`: a permutation gives the same bits (else the rule of assert_close); `alone_bitwise`: so does the member alone
    (the kernel does not depend on B)."""

    def __init__(self, name, fn, args, tables, members, env=None, bitwise=True, alone_bitwise=True):
        self.name, self.fn, self.args, self.tables, self.members = name, fn, args, tables, members
        self.env, self.bitwise, self.alone_bitwise = env or {}, bitwise, alone_bitwise

    def poisoned(self, kind):
        out = dict(self.args)
        for names, count, keep, what in self.tables:
            new = cc.poison([self.args[n] for n in names], self.args[count], kind,
                            None if keep is None else self.args[keep], what=what)
            out.update(dict(zip(names, new)))
        return out

    def permuted(self, perm, args=None):
        args = self.args if args is None else args
        return {k: (np.ascontiguousarray(v[perm]) if k in self.members else v) for k, v in args.items()}

    @property
    def B(self):
        return len(self.args[self.members[0]])


def check_padding(case):
    """(a) for one case."""
    with switches(case.env):
        zero = case.poisoned("zero")
        want = run(case.fn, zero, True)
        assert_same(run(case.fn, zero, True), want, (case.name, "not reproducible"))
        for kind in ("nan", "huge", "cut"):
            assert_same(run(case.fn, case.poisoned(kind), True), want, (case.name, kind, "device pointers"))
        want_h = run(case.fn, zero, False)
        assert_same(run(case.fn, case.poisoned("cut"), False), want_h, (case.name, "cut", "host pointers"))
    return want


def check_members(case, want, alone=(0,)):
    """(c) for one case: reversed, rolled by 3, and members alone; on "cut" padding."""
    B = case.B
    base = case.poisoned("cut")
    same = assert_same if case.bitwise else assert_close
    with switches(case.env):
        for perm in (np.arange(B)[::-1], np.roll(np.arange(B), 3)):
            got = run(case.fn, case.permuted(perm, base), True)
            same(got, {k: v[perm] for k, v in want.items()}, (case.name, "permuted"))
        for p in alone:
            one = {k: (np.ascontiguousarray(v[p:p + 1]) if k in case.members else v) for k, v in base.items()}
            got = run(case.fn, one, True)
            (assert_same if case.alone_bitwise else assert_close)(got, {k: v[p:p + 1] for k, v in want.items()},
                                                                  (case.name, "alone", p))


# ------------------------------------------------------------------------------------------------ the entry points, raw
class Fresh(batch._Backend):
    """The backend of one raw call, with every output filled with the byte 0xA5 first: a slot that a kernel leaves
    unwritten (a vertex slot beyond count, the x of an infeasible LP) compares as that pattern in every call, not as what
    the allocator left there from the call before."""

    def out(self, shape, dtype=np.float64, zero=False):
        o = super().out(shape, dtype, zero)
        if self.torch is None:
            o.view(np.uint8).fill(0xA5)
        elif o.numel():
            o.view(self.torch.uint8).fill_(0xA5)
        return o


def raw_lp(c, G, h, m):
    be = Fresh(G)
    B, m_max, n = G.shape
    res = dict(x=be.out((B, n)), fun=be.out((B,)), status=be.out((B,), np.int32), iters=be.out((B,), np.int32))
    be.call("plp_lp_solve_batch", B, m_max, n, c, G, h, m, res["x"], res["fun"], res["status"], res["iters"])
    return res


def raw_cheby(A, b, m):
    be = Fresh(A)
    B, m_max, d = A.shape
    res = dict(r=be.out((B,)), xc=be.out((B, d)), status=be.out((B,), np.int32))
    be.call("plp_cheby_batch", B, m_max, d, A, b, m, res["r"], res["xc"], res["status"])
    return res


def raw_bbox(A, b, m):
    be = Fresh(A)
    B, m_max, d = A.shape
    res = dict(lb=be.out((B, d)), ub=be.out((B, d)), status=be.out((B,), np.int32))
    be.call("plp_bbox_batch", B, m_max, d, A, b, m, res["lb"], res["ub"], res["status"])
    return res


def raw_reduce(A, b, m):
    be = Fresh(A)
    B, m_max, d = A.shape
    wide = m_max > 64
    res = dict(keep=be.out((B, (m_max + 63) // 64) if wide else (B,), np.uint64), flags=be.out((B,), np.int32),
               r=be.out((B,)), xc=be.out((B, d)), nlp=be.out((B,), np.int32))
    be.call("plp_reduce_wide_batch" if wide else "plp_reduce_batch", B, m_max, d, A, b, m, 1e-7, res["keep"], res["flags"],
            res["r"], res["xc"], res["nlp"])
    return res


def raw_contains(A, b, m, X, mode):
    be = Fresh(A)
    P, m_max, d = A.shape
    N = X.shape[1]
    out = be.out((P, N) if mode else (N,), np.uint8)
    be.call("plp_contains", P, m_max, d, A, b, m, N, X, 1e-7, mode, out)
    return dict(out=out)


def raw_pairs(A, b, m, n1):
    """The four pair entry points on one table: adjacency (full and the pairs 3 .. npairs - 2), overlap, and the cross
    pairs of the first n1 cells with the rest."""
    be = Fresh(A)
    n, m_max, d = A.shape
    npairs = n * (n - 1) // 2
    lo, hi = min(3, npairs), max(min(3, npairs), npairs - 2)
    res = dict(adj=be.out((n, n), np.uint8), rng=be.out((hi - lo,), np.uint8), ov=be.out((n, n), np.uint8),
               cross=be.out((n1, n - n1), np.uint8))
    be.call("plp_adjacent_pairs", n, m_max, d, A, b, m, 1e-7, res["adj"])
    if hi > lo:
        be.call("plp_adjacent_pairs_range", n, m_max, d, A, b, m, 1e-7, lo, hi, res["rng"])
    be.call("plp_overlap_pairs", n, m_max, d, A, b, m, 1e-7, res["ov"])
    be.call("plp_overlap_cross", n1, n - n1, m_max, d, A, b, m, 1e-7, res["cross"])
    return res


def raw_fm(A, b, m, keep, flags, col, first, mo_max):
    be = Fresh(A)
    B, m_max, d = A.shape
    kw = 0 if keep is None else 1
    head = (B, m_max, d, A, b, m, keep, kw, flags, col, first, 1e-7)
    res = dict(count=be.out((B,), np.int32), Ao=be.out((B, mo_max, d - 1 if col >= 0 else d)), bo=be.out((B, mo_max)),
               mo=be.out((B,), np.int32))
    be.call("plp_fm_count", *head, res["count"])
    be.call("plp_fm_emit", *head, mo_max, res["Ao"], res["bo"], res["mo"])
    return res


def raw_volume(A, b, m, lb, ub, state, inc, N):
    be = Fresh(A)
    B, m_max, d = A.shape
    res = dict(hits=be.out((B,), np.uint32), flags=be.out((B,), np.int32))
    be.call("plp_volume_hits", B, m_max, d, A, b, m, lb, ub, state, inc, N, res["hits"], res["flags"])
    return res


def raw_support(A, b, m, Cd, shared, xc):
    be = Fresh(A)
    B, m_max, d = A.shape
    K = Cd.shape[-2]
    res = dict(h=be.out((B, K)), x=be.out((B, K, d)), status=be.out((B, K), np.int32))
    be.call("plp_support_batch", B, m_max, d, A, b, m, K, Cd, shared, xc, res["h"], res["x"], res["status"])
    return res


def raw_extreme(A, b, m, keep, v_max):
    be = Fresh(A)
    B, m_max, d = A.shape
    res = dict(V=be.out((B, v_max, d)), count=be.out((B,), np.int32), basis=be.out((B, v_max, d), np.int32),
               status=be.out((B,), np.int32))
    be.call("plp_extreme_batch", B, m_max, d, A, b, m, keep, v_max, res["V"], res["count"], res["basis"], res["status"])
    return res


def raw_hull(X, n, keep, f_max):
    be = Fresh(X)
    B, n_max, d = X.shape
    res = dict(A=be.out((B, f_max, d)), b=be.out((B, f_max)), on=be.out((B, f_max), np.uint64), count=be.out((B,), np.int32),
               basis=be.out((B, f_max, d), np.int32), status=be.out((B,), np.int32))
    be.call("plp_hull_batch", B, n_max, d, X, n, keep, f_max, res["A"], res["b"], res["on"], res["count"], res["basis"],
            res["status"])
    return res


ROWS = [(("A", "b"), "m", None, "rows")]


def _case(name, fn, args, tables=ROWS, members=("A", "b", "m"), env=None, bitwise=True, alone_bitwise=True):
    return Case(name, fn, args, tables, members, env, bitwise, alone_bitwise)


# ------------------------------------------------------------------------------------------------ the cases
# the fused reduce: (m_max, d, switches, engine, gs / nw it must get at B = 257)
REDUCE = [
    (16, 3, {"PLP_REDUCE_1ROW": 1}, "GENERAL", None),
    (16, 10, {"PLP_REDUCE_R2": 0}, "GENERAL", None),
    (16, 3, {}, "LANE", 16),
    (16, 3, {"PLP_REDUCE_LANE_GS": 8}, "LANE", 8),
    (16, 3, {"PLP_REDUCE_LANE_GS": 4}, "LANE", 4),
    (24, 3, {}, "LANE", 16),
    (24, 4, {"PLP_REDUCE_LANE": 1, "PLP_REDUCE_LANE_GS": 8}, "LANE", 8),
    (16, 3, {"PLP_REDUCE_SPLIT": 0, "PLP_REDUCE_HALF": 0}, "GROUP", 4),
    (16, 6, {"PLP_REDUCE_SPLIT": 0}, "GROUP", 8),
    (16, 3, {"PLP_REDUCE_SPLIT": 0}, "GROUP_MIX", 4),
    (16, 3, {"PLP_REDUCE_LANE": 0}, "SPLIT", 4),
    (48, 6, {"PLP_REDUCE_WSPLIT": 0}, "WDENSE", 64),
    (48, 6, {"PLP_REDUCE_WDENSE": 0}, "LAZY", 64),
    (48, 14, {"PLP_REDUCE_WSPLIT": 0}, "LAZY", 64),
    (48, 6, {"PLP_REDUCE_WSPLIT": 2}, "WSPLIT", 2),
    (16, 6, {}, "WSPLIT", 4),
    (48, 14, {}, "WSPLIT", 4),
]
# engines only a default threshold reaches: (B, m_max, d, switches, engine); no reference per member
REDUCE_LARGE = [
    (16001, 24, 3, {}, "LANE_MIX"),
    (40001, 16, 3, {}, "LANE_MIX"),
    (70000, 16, 3, {"PLP_REDUCE_LANE": 0}, "GROUP_MIX"),
]
# The engines whose workgroups take members in turn (p, then p + gridDim.x, in the same LDS): fm_kernel, lp_lds_kernel,
# cheby_lds_kernel, reduce_lds_kernel.  Their launchers (launch_fm_t of plp_fm.hip, lds_grid of plp_lds.hip) start at most
# 256 CUs x 32 workgroups x 4 = 32 768 workgroups, fewer where the LDS of one member lets fewer share a CU; with more
# members than that every workgroup that holds one of the last 257 has held another before it.
GRID_CAP = 256 * 32 * 4
STRIDE_B = GRID_CAP + 257
STRIDE_ALONE = (0, 5, GRID_CAP + 5, STRIDE_B - 1)
REQUIRED = {("GENERAL", 0), ("LANE", 4), ("LANE", 8), ("LANE", 16), ("LANE_MIX", 0), ("GROUP", 0), ("GROUP_MIX", 0),
            ("SPLIT", 0), ("WDENSE", 0), ("LAZY", 0), ("WSPLIT", 2), ("WSPLIT", 4)}

LP = [   # (m_max, n, switches)
    (16, 3, {}), (16, 3, {"PLP_LP_1ROW": 1}), (24, 8, {}), (24, 8, {"PLP_LP_WIDE": 0}), (40, 17, {}), (70, 4, {}),
    (16, 3, {"PLP_LDS": 1}),
]
CHEBY = [(16, 3, {}), (16, 3, {"PLP_CHEBY_1ROW": 1}), (24, 9, {}), (24, 9, {"PLP_CHEBY_WIDE": 0}), (70, 4, {})]
BBOX = [
    (16, 3, {}), (16, 3, {"PLP_BBOX_LANE": 0}), (16, 3, {"PLP_BBOX_LANE": 0, "PLP_BBOX_SPLIT": 0}), (24, 6, {}),
    (24, 6, {"PLP_BBOX_WIDE": 1, "PLP_BBOX_WDENSE": 1}), (24, 6, {"PLP_BBOX_WIDE": 1, "PLP_BBOX_WDENSE": 0}),
    (24, 6, {"PLP_BBOX_WIDE": 0, "PLP_BBOX_SPLIT": 0}), (40, 14, {}),
    (24, 6, {"PLP_BBOX_WIDE": 1, "PLP_BBOX_WSPLIT": 0}), (40, 14, {"PLP_BBOX_WSPLIT": 0}),   # one wavefront per polytope
]
PAIRS = [(6, 2, {}), (10, 4, {}), (20, 8, {"PLP_ADJ_WIDE": 0}), (14, 5, {}), (28, 12, {})]   # (m_max, d, switches)
# What the plan of the LP family (plp_lp_plan.hpp) must say the lists above reach, at the sizes the tests run them:
# lp (engine, rows per lane, the phase-1 kernel follows), cheby (engine, rows per lane), bbox (engine, wavefronts per
# polytope, stored dictionary), pairs (engine, lanes per pair)
LP_REQUIRED = {
    "lp": {("LDS", 1, 0), ("WIDE", 1, 0), ("GROUP", 4, 1), ("GROUP", 4, 0), ("GROUP", 2, 0), ("GENERAL", 1, 0)},
    "cheby": {("LDS", 1), ("WIDE", 1), ("GROUP", 4), ("GROUP", 2), ("GENERAL", 1)},
    "bbox": {("LANE", 0, 0), ("SPLIT", 0, 0), ("GROUP", 0, 0), ("WIDE", 4, 1), ("WIDE", 4, 0), ("WIDE", 1, 1), ("WIDE", 1, 0)},
    "pairs": {("GROUP", 4), ("GROUP", 8), ("GROUP", 16), ("WIDE", 64)},
}
ENUM_SHAPES = [(5, 2), (16, 3), (12, 4), (64, 2)]
# (m_max, d, K): 16 / 32 / 64 row slots at K = 5 (8 lanes and 8 polytopes per workgroup), and the other steps of
# support::polytopes_per_group: K = 1 (one lane each: 64 per workgroup, 16 at 64 row slots, where np_cap holds), K = 33
# (a second tile of objectives, one polytope per workgroup)
SUPPORT_SHAPES = [(7, 2, 5), (16, 3, 5), (20, 4, 5), (40, 3, 5), (16, 3, 1), (40, 3, 1), (16, 3, 33)]


def ids(cases):
    return ["%s-%s-%s" % (c[0], c[1], ",".join("%s=%s" % (k[4:], v) for k, v in sorted(c[2].items())) or "default") for c in cases]


def rows_args(B, m_max, d, seed, min_m=1):
    A, b, m = cc.mixed_rows(B, m_max, d, seed, min_m=min_m)
    return dict(A=A, b=b, m=m)


def lp_args(B, m_max, n, seed):
    """Mixed LPs: member 1 has no rows (status 3), member 5 no rows and a zero cost (status 0)."""
    G, h, m = cc.mixed_rows(B, m_max, n, seed, min_m=0)
    c = np.random.default_rng(seed + 1).standard_normal((B, n))
    if B > 5:
        m[5] = 0
        G[5], h[5], c[5] = 0.0, 0.0, 0.0
    return dict(c=c, G=G, h=h, m=m)


LP_TABLES = [(("G", "h"), "m", None, "rows")]
LP_MEMBERS = ("c", "G", "h", "m")


@pytest.fixture(scope="module")
def plan(reduce_plan):
    """The plan of tests/test_reduce_plan.py, asked with the switches as the environment spells them -> dict by FIELDS."""
    def ask(B, m, d, env):
        return dict(zip(FIELDS, reduce_plan(B, m, d, {k[len("PLP_REDUCE_"):]: str(v) for k, v in env.items()})))
    return ask


# ------------------------------------------------------------------------------------------------ a + c: the LP family
def test_engine_coverage(plan):
    """The reduce cases below reach every engine of the plan, at the tile shapes asked for; the large ones do get the
    position-dependent forms (full tiles followed by short ones)."""
    seen = set()
    for m_max, d, env, engine, shape in REDUCE:
        got = plan(257, m_max, d, env)
        assert got["engine"] == engine, (m_max, d, env, got)
        if engine == "LANE":
            assert got["gs"] == shape
        if engine == "WSPLIT":
            assert got["nw"] == shape
        seen.add((engine, got["gs"] if engine == "LANE" else got["nw"] if engine == "WSPLIT" else 0))
    for B, m_max, d, env, engine in REDUCE_LARGE:
        got = plan(B, m_max, d, env)
        assert got["engine"] == engine and 0 < got["nbig"] < got["grid"], (B, m_max, d, got)
        seen.add((engine, 0))
    assert seen >= REQUIRED, REQUIRED - seen
    assert {ENGINES.index(e) for e, _ in REQUIRED} == set(range(1, len(ENGINES)))


def test_lp_engine_coverage(lp_plan):
    """The LP, CHEBY, BBOX and PAIRS cases below reach every engine of the LP family's plan, in each of its forms, at the
    sizes the tests run them (the pair calls: the matrix, the range 3 .. npairs - 2 and the cross pairs of raw_pairs)."""
    def ask(call, sizes, env):
        launches, _ = lp_plan(call, sizes, {k[len("PLP_"):]: str(v) for k, v in env.items()})
        assert launches, (call, sizes, env)
        return launches
    seen = {call: set() for call in LP_REQUIRED}
    for B in SIZES:
        for m_max, n, env in LP:
            L = ask("lp", (B, m_max, n), env)
            seen["lp"].add((L[0]["engine"], L[0]["rows"], int(len(L) == 3)))
            assert len(L) == 1 or (L[0]["engine"], L[-1]["engine"]) == ("GROUP", "GENERAL")
        for m_max, d, env in CHEBY:
            L = ask("cheby", (B, m_max, d), env)[0]
            seen["cheby"].add((L["engine"], L["rows"]))
        for m_max, d, env in BBOX:
            L = ask("bbox", (B, m_max, d), env)[0]
            seen["bbox"].add((L["engine"], L["nw"], L["dense"]))
    for n in (5, 20, 257):
        npairs, n1 = n * (n - 1) // 2, n // 3 + 1
        for m_max, d, env in PAIRS:
            for sizes in ((n, m_max, d, 0, 0, 0, 0), (n, m_max, d, 3, npairs - 2, 1, 0), (n, m_max, d, 0, n1 * (n - n1), 1, n1)):
                L = ask("pairs", sizes, env)[0]
                seen["pairs"].add((L["engine"], L["gs"]))
    for call, want in LP_REQUIRED.items():
        assert seen[call] >= want, (call, want - seen[call])
    assert {e[0] for want in LP_REQUIRED.values() for e in want} == set(LP_ENGINES) - {"NONE", "EMPTY"}


@pytest.mark.parametrize("m_max,d,env,engine,shape", REDUCE, ids=ids(REDUCE))
def test_reduce_padding_members_oracle(plan, oracle, m_max, d, env, engine, shape):
    for B in SIZES:
        mix = plan(B, m_max, d, env)["engine"] in ("LANE_MIX", "GROUP_MIX")
        case = _case("reduce %s B=%d" % (engine, B), raw_reduce, rows_args(B, m_max, d, seed=7 * m_max + d + B),
                     env=env, bitwise=not mix, alone_bitwise=False)
        want = check_padding(case)
        assert not (batch.keep_to_bool(want["keep"], m_max) & cc._dead(case.args["m"], m_max, None)).any()
        if B > 1:
            check_members(case, want, alone=(0, 2, 3, 4, B - 1) if B == 257 else ())
        if B == 257:
            reduce_vs_oracle(oracle, case.poisoned("cut"), want, 200)


def reduce_vs_oracle(oracle, args, got, count):
    A, b, m = args["A"], args["b"], args["m"]
    masks = batch.keep_to_bool(got["keep"], A.shape[1])
    for k in range(min(count, len(m))):
        o = oracle.reduce(A[k, :m[k]], b[k, :m[k]])
        assert int(got["flags"][k]) == o["flags"], (k, int(got["flags"][k]), o["flags"])
        assert np.array_equal(masks[k, :m[k]], o["keep"]), (k, masks[k, :m[k]], o["keep"])
        assert abs(got["r"][k] - o["r"]) <= TOL and int(got["nlp"][k]) == o["nlp"], k


@pytest.mark.parametrize("B,m_max,d,env,engine", REDUCE_LARGE, ids=["%s-%d" % (c[4], c[0]) for c in REDUCE_LARGE])
def test_reduce_large_batches_padding_and_members(B, m_max, d, env, engine):
    """The tile shape of a member depends on its position here: verdicts exact, the ball to the rule of _same."""
    case = _case("reduce %s B=%d" % (engine, B), raw_reduce, rows_args(B, m_max, d, seed=B), env=env, bitwise=False,
                 alone_bitwise=False)
    want = check_padding(case)
    check_members(case, want, alone=(0, B - 1))


def test_reduce_wide_padding_members_oracle(oracle):
    """(The oracle on the first 40 members: its reduce of 70 rows is some 70 LPs of 70 rows, one member at a time.)"""
    for B in SIZES:
        case = _case("reduce wide B=%d" % B, raw_reduce, rows_args(B, 70, 3, seed=70 + B), alone_bitwise=False)
        want = check_padding(case)
        assert want["keep"].shape == (B, 2)
        if B > 1:
            check_members(case, want, alone=(0, 2, 3, 4, B - 1) if B == 257 else ())
        if B == 257:
            reduce_vs_oracle(oracle, case.poisoned("cut"), want, 40)


def test_reduce_wide_members_in_turn():
    """reduce_lds_kernel with more members than workgroups: dictionary, rows and keep words in the LDS of the one before."""
    case = _case("reduce wide B=%d" % STRIDE_B, raw_reduce, rows_args(STRIDE_B, 70, 3, seed=7000), alone_bitwise=False)
    check_members(case, check_padding(case), alone=STRIDE_ALONE)


def test_lp_lds_members_in_turn():
    """lp_lds_kernel (PLP_LDS=1 at 16 rows: the kernel of the batches beyond 64) with more members than workgroups."""
    case = _case("lp LDS B=%d" % STRIDE_B, raw_lp, lp_args(STRIDE_B, 16, 3, seed=1600), LP_TABLES, LP_MEMBERS,
                 {"PLP_LDS": 1}, alone_bitwise=False)
    check_members(case, check_padding(case), alone=STRIDE_ALONE)


def test_cheby_lds_members_in_turn():
    case = _case("cheby LDS B=%d" % STRIDE_B, raw_cheby, rows_args(STRIDE_B, 16, 3, seed=1601), env={"PLP_LDS": 1},
                 alone_bitwise=False)
    check_members(case, check_padding(case), alone=STRIDE_ALONE)


@pytest.mark.parametrize("m_max,n,env", LP, ids=ids(LP))
def test_lp_padding_members_oracle(oracle, m_max, n, env):
    for B in SIZES:
        case = _case("lp B=%d" % B, raw_lp, lp_args(B, m_max, n, seed=11 * m_max + n + B), LP_TABLES, LP_MEMBERS, env,
                     alone_bitwise=False)
        want = check_padding(case)
        if B > 1:
            check_members(case, want, alone=(0, 1, 2, 3, 4, 5, B - 1) if B == 257 else ())
        if B == 257:
            assert want["status"][1] == 3 and want["status"][5] == 0 and {0, 2, 3} <= set(want["status"].tolist())
            a = case.poisoned("cut")
            for k in range(200):
                mk = a["m"][k]
                so, _, fo, _ = oracle.lp_solve(a["c"][k], a["G"][k, :mk], a["h"][k, :mk])
                assert want["status"][k] == so, (k, want["status"][k], so)
                if so == 0:
                    assert abs(want["fun"][k] - fo) <= TOL * max(1.0, abs(fo)), k
                    assert mk == 0 or np.max(a["G"][k, :mk] @ want["x"][k] - a["h"][k, :mk]) <= 1e-7


@pytest.mark.parametrize("m_max,d,env", CHEBY, ids=ids(CHEBY))
def test_cheby_padding_members_oracle(oracle, m_max, d, env):
    for B in SIZES:
        case = _case("cheby B=%d" % B, raw_cheby, rows_args(B, m_max, d, seed=13 * m_max + d + B), env=env,
                     alone_bitwise=False)
        want = check_padding(case)
        if B > 1:
            check_members(case, want, alone=(0, 1, 2, 3, 4, B - 1) if B == 257 else ())
        if B == 257:
            a = case.poisoned("cut")
            for k in range(200):
                mk = a["m"][k]
                so, ro, _ = oracle.cheby(a["A"][k, :mk], a["b"][k, :mk])
                assert want["status"][k] == so, (k, want["status"][k], so)
                if so == 0:
                    assert abs(want["r"][k] - ro) <= TOL, (k, want["r"][k], ro)
                    nrm = np.linalg.norm(a["A"][k, :mk], axis=1)
                    assert np.max(a["A"][k, :mk] @ want["xc"][k] + nrm * want["r"][k] - a["b"][k, :mk]) <= 1e-9


@pytest.mark.parametrize("m_max,d,env", BBOX, ids=ids(BBOX))
def test_bbox_padding_members_oracle(oracle, m_max, d, env):
    """Against the oracle with the rule of test_gpu_parity.test_bbox_vs_oracle: boxes to 1e-9 with +-inf in the same
    places; handed back (status 1) exactly where there is no centre with r >= 1e-6."""
    for B in SIZES:
        case = _case("bbox B=%d" % B, raw_bbox, rows_args(B, m_max, d, seed=17 * m_max + d + B), env=env,
                     alone_bitwise=False)
        want = check_padding(case)
        if B > 1:
            check_members(case, want, alone=(0, 1, 2, 3, 4, B - 1) if B == 257 else ())
        if B == 257:
            a = case.poisoned("cut")
            for k in range(200):
                mk = a["m"][k]
                lb, ub, bad = oracle.bounding_box(a["A"][k, :mk], a["b"][k, :mk])
                r, _ = oracle.cheby_ball(a["A"][k, :mk], a["b"][k, :mk])
                if want["status"][k] == 0:
                    assert bad == 0 and r >= 1e-6 - 1e-12, (k, r)
                    assert np.allclose(want["lb"][k], lb.ravel(), rtol=0, atol=TOL), (k, want["lb"][k], lb.ravel())
                    assert np.allclose(want["ub"][k], ub.ravel(), rtol=0, atol=TOL), (k, want["ub"][k], ub.ravel())
                else:   # (d > 8: the header also hands back LPs of more than 32 pivots)
                    assert want["status"][k] == 1 and (r < 1e-6 + 1e-12 or d > 8), (k, r)
            assert (want["status"] == 0).sum() > 128 or d > 8


# ------------------------------------------------------------------------------------------------ a + c + d: contains, pairs
@pytest.mark.parametrize("m_max,d", [(16, 3), (16, 6), (40, 2)])
def test_contains_padding_members_oracle(oracle, m_max, d):
    X = np.random.default_rng(d).uniform(-3.5, 3.5, (d, 1000))
    for P in SIZES:
        a = rows_args(P, m_max, d, seed=19 * m_max + d + P)
        for mode in (1, 0):
            case = _case("contains P=%d mode=%d" % (P, mode), raw_contains, dict(a, X=X, mode=mode))
            want = check_padding(case)
            if mode == 1 and P > 1:
                check_members(case, want, alone=(0, 2, P - 1) if P == 257 else ())
            if P > 1:
                live = case.poisoned("cut")
                ref = np.stack([oracle.contains(live["A"][p:p + 1, :a["m"][p]], live["b"][p:p + 1, :a["m"][p]],
                                                np.ascontiguousarray(X.T))[0] for p in range(min(P, 200))])
                if mode == 1:
                    assert np.array_equal(want["out"][:len(ref)], ref)
                    assert 0 < ref.sum() < ref.size
                elif P <= 200:
                    assert np.array_equal(want["out"], ref.any(axis=0).astype(np.uint8))


def cells(n, m_max, d, seed):
    """n ragged random cells: boxes with random centres and widths (overlapping, apart) cut by random half-spaces.  With
    n >= 5: cell 1 is empty (x_0 <= c, x_0 >= c + 1), cell 2 flat and not empty (x_0 = c inside its box: a neighbour once
    its rows are inflated, never an overlap), cell 3 unbounded (the d upper sides of its box only).  With n >= 7 also:
    cell 5 empty by a zero row with b = -1, cell 6 unbounded like cell 3 (the pair (6, 3) is an unbounded LP)."""
    rng = np.random.default_rng(seed)
    cen, hw = rng.uniform(0.0, 2.0, (n, d)), rng.uniform(0.3, 0.9, (n, d))
    A, b = np.zeros((n, m_max, d)), np.zeros((n, m_max))
    A[:, :d], A[:, d:2 * d] = np.eye(d), -np.eye(d)
    b[:, :d], b[:, d:2 * d] = cen + hw, -(cen - hw)
    extra = rng.standard_normal((n, m_max - 2 * d, d))
    extra /= np.linalg.norm(extra, axis=2, keepdims=True)
    A[:, 2 * d:] = extra
    b[:, 2 * d:] = np.einsum("nij,nj->ni", extra, cen) + rng.uniform(0.2, 1.5, (n, m_max - 2 * d))
    m = rng.integers(2 * d, m_max + 1, n).astype(np.int32)
    m[0] = m_max
    j, e0 = 2 * d, np.eye(d)[0]
    if n >= 5:
        A[1, j], A[1, j + 1], b[1, j], b[1, j + 1] = e0, -e0, cen[1, 0], -cen[1, 0] - 1.0
        A[2, j], A[2, j + 1], b[2, j], b[2, j + 1] = e0, -e0, cen[2, 0], -cen[2, 0]
        m[1], m[2], m[3] = max(m[1], j + 2), max(m[2], j + 2), d
    if n >= 7:
        A[5, j], b[5, j] = 0.0, -1.0
        m[5], m[6] = max(m[5], j + 1), d
    for p in range(n):
        A[p, m[p]:], b[p, m[p]:] = 0.0, 0.0
    return dict(A=A, b=b, m=m)


def pair_matrices(res, n, n1):
    """The four outputs as symmetric n x n matrices with -1 where an output says nothing about the pair."""
    ii, jj = np.tril_indices(n, -1)
    npairs = len(ii)
    lo, hi = min(3, npairs), max(min(3, npairs), npairs - 2)
    rng = -np.ones((n, n), np.int16)
    rng[ii[lo:hi], jj[lo:hi]] = res["rng"]
    rng[jj[lo:hi], ii[lo:hi]] = res["rng"]
    cross = -np.ones((n, n), np.int16)
    cross[:n1, n1:] = res["cross"]
    cross[n1:, :n1] = res["cross"].T
    return dict(adj=res["adj"].astype(np.int16), rng=rng, ov=res["ov"].astype(np.int16), cross=cross)


@pytest.mark.parametrize("m_max,d,env", PAIRS, ids=ids(PAIRS))
def test_pairs_padding_members_oracle(oracle, m_max, d, env):
    """The pair kernels on ragged random cells (d = 2 .. 4 among them).  Against the oracle with the rule of
    test_gpu_parity's by_cheby: the Chebyshev LP of the stacked live rows, b + abs_tol and r > abs_tol / 10 for adjacency,
    b and r > abs_tol for overlap, no where the oracle's status is not 0 (an empty or an unbounded stack); no pair of these
    cells comes within 1e-9 of either threshold (asserted).  Padding, permutations and a pair alone at 5, 20 and 257
    cells; the oracle on every pair of 5 and of 20."""
    tol = 1e-7
    for n in (5, 20, 257):
        n1 = n // 3 + 1
        case = _case("pairs n=%d" % n, raw_pairs, dict(cells(n, m_max, d, seed=23 * m_max + d + n), n1=n1), env=env)
        want = check_padding(case)
        W = pair_matrices(want, n, n1)
        assert np.array_equal(W["adj"], W["adj"].T) and np.all(np.diag(W["adj"]) == 1)
        a = case.poisoned("cut")
        with switches(env):
            for perm in (np.arange(n)[::-1], np.roll(np.arange(n), 3)):
                G = pair_matrices(run(raw_pairs, case.permuted(perm, a), True), n, n1)
                for k in ("adj", "ov"):
                    assert np.array_equal(G[k], W[k][np.ix_(perm, perm)]), (k, n)
                for k in ("rng", "cross"):   # another slice of the pair space: equal wherever both say something
                    both = (G[k] >= 0) & (W[k][np.ix_(perm, perm)] >= 0)
                    assert np.array_equal(G[k][both], W[k][np.ix_(perm, perm)][both]) and both.any(), (k, n)
            for i, j in ((4, 0), (3, 2), (2, 1), (n - 1, 3), (n - 1, n - 2)):
                two = {k: (np.ascontiguousarray(v[[i, j]]) if k in case.members else v) for k, v in a.items()}
                alone = run(raw_pairs, dict(two, n1=1), True)
                assert alone["adj"][0, 1] == want["adj"][i, j] and alone["ov"][0, 1] == want["ov"][i, j], (i, j)
                assert alone["cross"][0, 0] == want["ov"][i, j], (i, j)
        # the special cells by what they are, at every size: nothing meets an empty cell, the flat one only touches
        assert not W["adj"][1, [0, 2, 3, 4]].any() and not W["ov"][1, [0, 2, 3, 4]].any()
        assert not W["ov"][2, [0, 1, 3, 4]].any()
        if n >= 7:
            assert not W["adj"][5, [0, 1, 2, 3, 4, 6]].any() and not W["adj"][6, 3] and not W["ov"][6, 3]
        near = 0
        for i in range(n if n <= 20 else 0):
            for j in range(i):
                SA = np.vstack([a["A"][i, :a["m"][i]], a["A"][j, :a["m"][j]]])
                Sb = np.hstack([a["b"][i, :a["m"][i]], a["b"][j, :a["m"][j]]])
                for key, inflate, thresh in (("adj", tol, tol / 10), ("ov", 0.0, tol)):
                    st, r, _ = oracle.cheby(SA, Sb + inflate)
                    assert st != 0 or abs(r - thresh) > 1e-9, (i, j, key, r)
                    yes = int(st == 0 and r > thresh)
                    assert W[key][i, j] == yes, (i, j, key, st, r)
                    near += yes
                    for k2 in (("rng",) if key == "adj" else ("cross",)):
                        assert W[k2][i, j] in (-1, yes), (i, j, k2)
        assert n != 20 or 0 < near < n * (n - 1)


# ------------------------------------------------------------------------------------------------ a + c: the newer entry points
@pytest.mark.parametrize("first", [0, 1], ids=["later", "first"])
@pytest.mark.parametrize("m_max,d", [(10, 3), (14, 4)])
def test_fm_padding_and_members(m_max, d, first):
    """plp_fm_count / plp_fm_emit with m alone and with the keep words and flags of a reduce of the same rows (rows whose
    keep bit is clear do not exist either), on the last column and without elimination."""
    for B in SIZES:
        a = rows_args(B, m_max, d, seed=29 * m_max + d + B)
        red = run(raw_reduce, a, True)
        keep, flags = red["keep"].view(np.uint64), red["flags"]
        for col in (d - 1, -1):
            for kp, fl in ((None, None), (keep, flags)):
                case, count = fm_case(a, kp, fl, col, first)
                want = check_padding(case)
                assert np.array_equal(want["count"], count) and (want["mo"] >= 0).all()
                if B > 1:
                    check_members(case, want, alone=(0, 2, B - 1) if B == 257 else ())
        assert count.max() > 0


def fm_case(a, keep, flags, col, first):
    """plp_fm_count + plp_fm_emit on the rows `a`, the output sized by the largest count -> (case, count)."""
    args = dict(a, keep=keep, flags=flags, col=col, first=first, mo_max=1)
    tables = [(("A", "b"), "m", None if keep is None else "keep", "rows")]
    members = ("A", "b", "m") + (("keep", "flags") if keep is not None else ())
    count = run(raw_fm, args, True)["count"]
    args["mo_max"] = max(1, int(count.max()))
    return _case("fm B=%d col=%d keep=%s" % (len(count), col, keep is not None), raw_fm, args, tables, members), count


@pytest.mark.parametrize("keep", [False, True], ids=["m", "keep"])
def test_fm_members_in_turn(keep):
    """More members than workgroups: fm_kernel takes member p + gridDim.x after member p, its rows and its P / Q / N lists
    in the LDS of the one before."""
    a = rows_args(STRIDE_B, 10, 3, seed=2900)
    red = run(raw_reduce, a, True) if keep else None
    case, count = fm_case(a, red["keep"].view(np.uint64) if keep else None, red["flags"] if keep else None, 2, 0)
    want = check_padding(case)
    assert np.array_equal(want["count"], count) and (want["mo"] >= 0).all() and len(set(count[GRID_CAP:].tolist())) > 3
    check_members(case, want, alone=STRIDE_ALONE)


@pytest.mark.parametrize("grid", [None, 7], ids=["tiles", "grid-stride"])
@pytest.mark.parametrize("d", [1, 3, 4])
def test_volume_padding_and_members(d, grid):
    """plp_volume_hits, N = 777 in the box [-3.1, 3.1]^d; m = 0 is VF_NOROWS.  grid-stride: a workgroup takes several
    (member, tile) items in turn."""
    env = {} if grid is None else {"PLP_VOLUME_MAX_GRID": grid}
    for B in SIZES:
        a = rows_args(B, 2 * d + 5, d, seed=31 + d + B, min_m=0)
        state, inc = batch._pcg64_words([1000 + p for p in range(B)])
        args = dict(a, lb=np.full((B, d), -3.1), ub=np.full((B, d), 3.1), state=state, inc=inc, N=777)
        case = _case("volume B=%d" % B, raw_volume, args, members=("A", "b", "m", "lb", "ub", "state", "inc"), env=env)
        want = check_padding(case)
        if B > 1:
            assert want["flags"][1] == batch.VF_NOROWS and want["hits"][1] == 0 and 0 < want["hits"][0] < 777
            check_members(case, want, alone=(0, 1, 2, B - 1) if B == 257 else ())


@pytest.fixture(scope="module")
def SL(tmp_path_factory):
    return sh.build(tmp_path_factory.mktemp("support_host"))


@pytest.mark.parametrize("shared", [1, 0], ids=["shared", "own"])
@pytest.mark.parametrize("m_max,d,K", SUPPORT_SHAPES)
def test_support_padding_members_oracle(oracle, SL, m_max, d, K, shared):
    """plp_support_batch from the origin: padding, permutations, members alone; where the kernel settles an LP
    (status 0 / 3) the oracle's simplex on the live rows agrees (support_host.check_against_oracle), on 200 members, 100
    at K = 33."""
    for B in SIZES:
        a = rows_args(B, m_max, d, seed=37 * m_max + d + B, min_m=0)
        Cd = np.random.default_rng(m_max + B).standard_normal((K, d) if shared else (B, K, d))
        args = dict(a, Cd=Cd, shared=shared, xc=np.zeros((B, d)))
        case = _case("support B=%d" % B, raw_support, args, members=("A", "b", "m", "xc") + (() if shared else ("Cd",)))
        want = check_padding(case)
        if B > 1:
            check_members(case, want, alone=(0, 1, 2, 3, 4, B - 1) if B == 257 else ())
        if B == 257:
            n = 200 if K <= 5 else 100
            live = case.poisoned("cut")
            Cn = Cd if shared else Cd[:n]
            ost, oh, ox = sh.oracle_support(oracle, live["A"][:n], live["b"][:n], a["m"][:n], Cn, extent=True)
            st = want["status"][:n]
            assert set(np.unique(st)) <= {0, 1, 3} and (st == 0).mean() > 0.8
            assert not np.any((ost == 3) & (st == 0)) and not np.any((ost == 0) & (st == 3))
            sh.check_against_oracle(live["A"][:n], live["b"][:n], a["m"][:n], Cn, want["h"][:n], want["x"][:n], st, ost, oh,
                                    where=(st != 1), ext=ox)


@pytest.mark.parametrize("m_max,d", ENUM_SHAPES)
def test_extreme_padding_and_members(m_max, d):
    for B in SIZES:
        a = rows_args(B, m_max, d, seed=41 * m_max + d + B, min_m=0)
        keep = cc.keep_words(np.random.default_rng(B), B, forced=d)
        for kp in (None, keep):
            args = dict(a, keep=kp, v_max=xh.vmax_for(d, m_max))
            case = _case("extreme B=%d" % B, raw_extreme, args, [(("A", "b"), "m", None if kp is None else "keep", "rows")],
                         ("A", "b", "m") + (("keep",) if kp is not None else ()))
            want = check_padding(case)
            if B > 1:
                assert want["status"][1] == xh.XS_EMPTY and (want["status"] == xh.XS_OK).any()
                check_members(case, want, alone=(0, 1, 2, 3, 4, B - 1) if B == 257 else ())


@pytest.mark.parametrize("n_max,d", ENUM_SHAPES)
def test_hull_padding_and_members(n_max, d):
    for B in SIZES:
        X, n = cc.mixed_points(B, n_max, d, seed=43 * n_max + d + B)
        keep = cc.keep_words(np.random.default_rng(B + 1), B, forced=d + 1)
        for kp in (None, keep):
            args = dict(X=X, n=n, keep=kp, f_max=hh.fmax_for(d, n_max))
            case = _case("hull B=%d" % B, raw_hull, args, [(("X",), "n", None if kp is None else "keep", "points")],
                         ("X", "n") + (("keep",) if kp is not None else ()))
            want = check_padding(case)
            if B > 1:
                assert want["status"][1] == hh.HS_FLAT and (want["status"] == hh.HS_OK).any()
                check_members(case, want, alone=(0, 1, 2, 3, 4, B - 1) if B == 257 else ())


# ------------------------------------------------------------------------------------------------ d: the exact references
@pytest.mark.parametrize("d", [2, 3, 4])
def test_hull_equals_the_exact_hull(d):
    """The lattice sets of tests/test_batch_contract_host.py through plp_hull_batch, host pointers and device pointers,
    with answer-changing padding; the assertions of the host test, no case left out."""
    sets = cc.lattice_sets(d, cc.HULL_CASES[d], seed=70 + d)
    X, n = cc.pack_points(sets)
    Xp, = cc.poison((X,), n, "cut", what="points")
    args = dict(X=Xp, n=n, keep=None, f_max=hh.fmax_for(d, X.shape[1]))
    res_h, res_d = run(raw_hull, args, False), run(raw_hull, args, True)
    assert_same(res_d, res_h, "hull: device pointers against host pointers")
    for k, pts in enumerate(sets):
        least = cc.check_hull(pts, res_h["A"][k], res_h["b"][k], res_h["on"][k], int(res_h["count"][k]), int(res_h["status"][k]))
        assert least >= cc.MIN_DISTANCE, (d, k, least)
    assert set(res_h["status"].tolist()) == {hh.HS_OK, hh.HS_FLAT}


@pytest.mark.parametrize("d", [2, 3, 4])
def test_extreme_equals_the_exact_vertices(d):
    cases = cc.integer_polytopes(d, cc.VERTEX_CASES[d], seed=80 + d)
    A, b, m = cc.pack_rows(cases)
    Ap, bp = cc.poison((A, b), m, "cut")
    args = dict(A=Ap, b=bp, m=m, keep=None, v_max=xh.vmax_for(d, A.shape[1]))
    res_h, res_d = run(raw_extreme, args, False), run(raw_extreme, args, True)
    assert_same(res_d, res_h, "extreme: device pointers against host pointers")
    for k, (Ak, bk) in enumerate(cases):
        least = cc.check_vertices(Ak, bk, res_h["V"][k], int(res_h["count"][k]), int(res_h["status"][k]), xh.MATCH)
        assert least >= cc.MIN_DISTANCE, (d, k, least)
    assert set(res_h["status"].tolist()) == {xh.XS_OK, xh.XS_EMPTY}


# ------------------------------------------------------------------------------------------------ b: the Python calls
def python_call(name, fn, args, tables, members=()):
    """(b) for one public call: zero padding twice, then NaN / 1e300 / cut as CUDA tensors and cut as numpy arrays."""
    case = _case(name, fn, args, tables, members)
    return check_padding(case)


def test_python_extreme_batch_reduce():
    for B in (5, 257):
        a = rows_args(B, 16, 3, seed=900 + B)
        want = python_call("extreme_batch", lambda A, b, m: batch.extreme_batch(A, b, m=m), a, ROWS)
        assert want["status"][0] == batch.XS_OK and want["count"][0] >= 4
        assert want["status"][3] == want["status"][4] == batch.XS_FLAT and want["status"][2] != batch.XS_OK


def test_python_volume_batch_own_boxes():
    for B in (5, 257):
        a = rows_args(B, 12, 3, seed=910 + B)
        seeds = list(range(B))
        want = python_call("volume_batch", lambda A, b, m: {k: v for k, v in batch.volume_batch(
            A, b, m=m, nsamples=500, seed=seeds).items() if k in ("volume", "hits", "lb", "ub", "flags")}, a, ROWS)
        assert want["flags"][0] == 0 and want["hits"][0] > 0 and want["flags"][3] != 0 and np.isnan(want["volume"][3])


def test_python_support_batch_resolve():
    """xc=None, resolve=True: the empty and the flat member have no centre and are handed back to lpsolve_batch."""
    Cd = np.random.default_rng(5).standard_normal((5, 3))
    for B in (5, 257):
        a = rows_args(B, 16, 3, seed=920 + B)
        want = python_call("support_batch", lambda A, b, m: batch.support_batch(A, b, Cd, m=m), a, ROWS)
        assert (want["status"][0] == 0).all() and (want["status"][3] == 2).all() and 3 in want["status"][2]


def test_python_subset_batch_beyond_mq():
    """Q = P blown up (P <= Q) or moved (not): rows of Q beyond mq[p] do not exist, rows of P beyond m[p] neither."""
    for B in (5, 257):
        A, b, m = cc.mixed_rows(B, 12, 3, seed=930 + B, bounded_only=True)
        rng = np.random.default_rng(B)
        mq = rng.integers(1, 13, B).astype(np.int32)
        QA, Qb = A.copy(), b * 1.5
        Qb[::2] = b[::2] - 1.5
        tables = [(("A", "b"), "m", None, "rows"), (("QA", "Qb"), "mq", None, "q")]
        args = dict(A=A, b=b, m=m, QA=QA, Qb=Qb, mq=mq)
        case = _case("subset_batch", lambda A, b, m, QA, Qb, mq: dict(sub=batch.subset_batch(A, b, QA, Qb, m=m, mq=mq)),
                     args, tables, ())
        out = {}
        for kind in cc.KINDS:
            p = dict(args)
            p["A"], p["b"] = cc.poison((A, b), m, kind)
            p["QA"], p["Qb"] = cc.poison((QA, Qb), mq, kind, what="q", violated_by=np.zeros((B, 3)))
            out[kind] = run(case.fn, p, True)["sub"]
            if kind in ("zero", "cut"):
                assert np.array_equal(run(case.fn, p, False)["sub"], out[kind]), kind
        for kind in cc.KINDS:
            assert np.array_equal(out[kind], out["zero"]), kind
        assert out["zero"].any() and not out["zero"].all()


def test_python_projection_batch_two_steps():
    saved, solvers.default_solver = solvers.default_solver, "hip"
    try:
        for B in (5, 257):
            A, b, m = cc.mixed_rows(B, 12, 4, seed=940 + B, bounded_only=True)
            want = python_call("projection_batch", lambda A, b, m: {k: v for k, v in batch.projection_batch(
                A, b, [1, 2], m=m).items() if k in ("A", "b", "m", "status")}, dict(A=A, b=b, m=m), ROWS)
            assert (want["status"] == 0).all() and want["A"].shape[2] == 2 and (want["m"] >= 3).all()
    finally:
        solvers.default_solver = saved


def test_python_hull_batch_fmax():
    for B in (5, 257):
        X, n = cc.mixed_points(B, 16, 3, seed=950 + B)
        n[0] = 12   # (f_max follows n.max(): no member uses all 16 slots)
        n = np.minimum(n, 12).astype(np.int32)
        want = python_call("hull_batch", lambda X, n: batch.hull_batch(X, n=n), dict(X=X, n=n), [(("X",), "n", None, "points")])
        assert want["A"].shape[1] == hh.fmax_for(3, 12) and want["status"][0] == batch.HS_OK
