"""GPU: every template instance the dispatch can launch -- fused reduce(), stand-alone LPs, Chebyshev balls, bounding boxes,
pair LPs -- runs once on a small batch, every member against the oracle.  One case per instance, from the census of
tests/instance_cases.py (profiles/kernel_instances.json; tests/test_kernel_instances_host.py holds that file equal to what
the plans can return).  Each case first asserts through the plan that the call it is about to make launches the instance in
its id, then makes it under the case's switches.

The batch of a case: the seven families of scripts/soak_lane.py: make (random, ragged, unbounded, dup, scaled, flat, lattice),
16 members each (the pair calls: 4 cells each), then `random` members where the instance needs a larger batch.

Rules, those of the suite:
  reduce        test_gpu_parity.py: test_soak_families_small -- keep mask and flags exact, r to 1e-9 relative, LP count equal
                or scripts/soak_lane.py: prefilter_tie; over the module at most one such count in a thousand differs
  cheby, bbox   the same test's -- status exact and r to 1e-9 relative; soak_lane.box_equal with hair_unbounded_tol on `dup`
  lp            test_fuzz_random_shapes -- status exact, value to 1e-9 max(1, |f|), random costs, every other feasible set moved
                off the origin; on `dup` scipy / HiGHS arbitrates as in scripts/soak_lp.py
  pairs         test_batch_contract_gpu.py: test_pairs_padding_members_oracle -- the Chebyshev LP of the stacked live rows
The large cases (reduce_lane_mix_kernel, the 8- and 4-lane tiles of bbox_lane_kernel: 14 001 .. 40 001 members): every member
against the same members run in chunks small enough for the 16-lane tile shape -- verdicts exact and the ball / the box to
rounding (test_reduce_lane_gpu.py: _same), every bit on the members of `unbounded`, whose rows are in general position and
do not tie -- and every 37th member against the oracle.

Found by these cases: pairs-adjacent_r_kernel<8,8>-B28-m16-ADJ_WIDE=0, cells (13, 4), and
pairs-adjacent_w_kernel<15>-B28-m32-default, cells (14, 4) -- a `dup` cell that lost sides of its box to copies of other rows,
stacked with a `ragged` cell of 5 / 1 rows: r = 2.0 / 3.0 by the oracle, HiGHS and the verified plp_cheby_batch, but every
engine ends the LP "unbounded" (pivots below its tolerance), and the pair calls took that for "no".  They now hand such pairs to
the careful engine (careful_pairs_kernel, plp_verify.hip)."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, "tests"), os.path.join(ROOT, "scripts")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import instance_cases as ic  # noqa: E402
import soak_lane as SL  # noqa: E402
from test_batch_contract_gpu import switches  # noqa: E402
from test_lp_plan import plan as lp_plan  # noqa: E402,F401 (a fixture: the compiled plan)
from test_reduce_lane_gpu import _same, _same_bits  # noqa: E402
from test_reduce_plan import plan as reduce_plan  # noqa: E402,F401 (likewise)

pytestmark = pytest.mark.gpu

TOL = 1e-9
ABS_TOL = 1e-7
LP_COUNTS = {"members": 0, "differ": 0}   # reduce, over the module: members against the oracle, LP counts excused by prefilter_tie


@pytest.fixture(scope="module")
def pa():
    import polytope_amd as pa
    from polytope_amd import _lib
    assert _lib.available(), "libplp_hip.so did not load or no gfx950 device: the HIP path is mandatory"
    return pa


@pytest.fixture(scope="module")
def plans(reduce_plan, lp_plan):  # noqa: F811
    return {"reduce": reduce_plan, "lp": lp_plan}


def device_call(fn, *arrays):
    """fn on CUDA copies of the arrays -> its outputs on the host"""
    import torch
    res = fn(*[torch.as_tensor(np.ascontiguousarray(a)).cuda() for a in arrays])
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in res.items()} if isinstance(res, dict) else res.cpu().numpy()


def run(pa, call, mem, lo=0, hi=None):
    from polytope_amd import batch
    sl = slice(lo, hi)
    A, b, m = mem["A"][sl], mem["b"][sl], mem["m"][sl]
    if call == "reduce":
        return device_call(pa.reduce_batch, A, b, m)
    if call == "cheby":
        return device_call(lambda A, b, m: pa.cheby_ball_batch(A, b, m=m), A, b, m)
    if call == "bbox":
        return device_call(pa.bbox_batch, A, b, m)
    if call == "lp":
        return device_call(pa.lpsolve_batch, mem["c"][sl], A, b, m)
    return dict(adj=device_call(lambda A, b, m: batch.adjacent_pairs(A, b, m, abs_tol=ABS_TOL), A, b, m),
                ov=device_call(lambda A, b, m: batch.overlap_pairs(A, b, m, abs_tol=ABS_TOL), A, b, m))


def rows_of(mem, k):
    return mem["A"][k, :mem["m"][k]], mem["b"][k, :mem["m"][k]]


def reduce_vs_oracle(oracle, got, mem, idx, what):
    keep = got["keep"].view(np.uint64)
    for k in idx:
        Ak, bk = rows_of(mem, k)
        o = oracle.reduce(Ak, bk)
        same = int(keep[k]) == int(o["mask"]) and int(got["flags"][k]) == int(o["flags"]) and \
            abs(got["r"][k] - o["r"]) <= TOL * max(1.0, abs(o["r"]))
        assert same, (what, mem["fam"][k], k, hex(int(keep[k])), hex(int(o["mask"])), int(got["flags"][k]), o["flags"], got["r"][k], o["r"])
        LP_COUNTS["members"] += 1
        if int(got["nlp"][k]) != int(o["nlp"]):
            assert SL.prefilter_tie(Ak, bk), (what, mem["fam"][k], k, int(got["nlp"][k]), o["nlp"])
            LP_COUNTS["differ"] += 1


def cheby_vs_oracle(oracle, got, mem, idx, what):
    for k in idx:
        so, ro, _ = oracle.cheby(*rows_of(mem, k))
        assert int(got["status"][k]) == so and (so != 0 or abs(got["r"][k] - ro) <= TOL * max(1.0, abs(ro))), \
            (what, mem["fam"][k], k, int(got["status"][k]), so, got["r"][k], ro)


def bbox_vs_oracle(oracle, got, mem, idx, what):
    for k in idx:
        if got["status"][k] != 0:
            continue
        lo, hi, bad = oracle.bounding_box(*rows_of(mem, k))
        hair = 1e-8 if mem["fam"][k] == "dup" else None
        assert bad == 0 and SL.box_equal(got["lb"][k], got["ub"][k], lo, hi, hair_unbounded_tol=hair), \
            (what, mem["fam"][k], k, got["lb"][k], lo, got["ub"][k], hi)


def lp_vs_oracle(oracle, got, mem, idx, what):
    from scipy.optimize import linprog
    for k in idx:
        (Gk, hk), ck = rows_of(mem, k), mem["c"][k]
        so, _x, fo, _it = oracle.lp_solve(ck, Gk, hk)
        st, fun = int(got["status"][k]), got["fun"][k]
        ok = st == so and (so != 0 or abs(fun - fo) <= TOL * max(1.0, abs(fo)))
        if not ok and mem["fam"][k] == "dup":   # rows a hair apart: HiGHS, called as solvers.py does, arbitrates (scripts/soak_lp.py)
            rs = linprog(ck, Gk, hk, None, None, bounds=(None, None))
            ok = rs.status == st and (rs.status != 0 or abs(rs.fun - fun) <= 1e-6 * max(1.0, abs(fun)))
        assert ok, (what, mem["fam"][k], k, st, so, fun, fo)


def pairs_vs_oracle(oracle, got, mem, what):
    n = len(mem["m"])
    assert np.array_equal(got["adj"], got["adj"].T) and np.all(np.diag(got["adj"]) == 1), what
    assert got["adj"].max() <= 1 and got["ov"].max() <= 1, what   # (no pair is left at the engines' "undecided" mark)
    yes = 0
    for i in range(n):
        for j in range(i):
            (Ai, bi), (Aj, bj) = rows_of(mem, i), rows_of(mem, j)
            SA, Sb = np.vstack([Ai, Aj]), np.hstack([bi, bj])
            for key, inflate, thresh in (("adj", ABS_TOL, ABS_TOL / 10), ("ov", 0.0, ABS_TOL)):
                st, r, _ = oracle.cheby(SA, Sb + inflate)
                assert st != 0 or abs(r - thresh) > 1e-9, (what, i, j, key, r)   # (the inputs: no pair on a threshold)
                want = int(st == 0 and r > thresh)
                assert got[key][i, j] == want and got[key][j, i] == want, (what, mem["fam"][i], mem["fam"][j], i, j, key, st, r)
                yes += want
    return yes


VS_ORACLE = {"reduce": reduce_vs_oracle, "cheby": cheby_vs_oracle, "bbox": bbox_vs_oracle, "lp": lp_vs_oracle}


def chunked_on_16_lanes(pa, plans, case, mem):
    """The members of a large case in equal chunks of at most PLP_REDUCE_LANE_GS16_MAXB (17 .. 32 rows:
    PLP_REDUCE_LANE32_GS16_MAXB) members, each of which the plan gives to the 16-lane tile shape of the same kernel family."""
    call, B, m_max, d, sw = case[:5]
    limit = max(b for b in ic.batch_sizes(plans, call) if b <= (14000 if m_max <= 16 else 16000))
    bounds = np.linspace(0, B, -(-B // limit) + 1).astype(int)
    parts = []
    for lo, hi in zip(bounds[:-1], bounds[1:]):
        want = "%s_lane_kernel<%d, 16, %d>" % ("reduce" if call == "reduce" else "bbox", d, 16 if m_max <= 16 else 32)
        assert ic.planned(plans, call, int(hi - lo), m_max, d, sw) == [want], (lo, hi)
        parts.append(run(pa, call, mem, lo, hi))
    return {k: np.concatenate([p[k] for p in parts]) for k in parts[0]}


@pytest.mark.parametrize("case", ic.CASES, ids=[ic.case_id(c) for c in ic.CASES])
def test_instance(pa, plans, oracle, case):
    call, B, m_max, d, sw, name, launches = case
    what = ic.case_id(case)
    assert ic.planned(plans, call, B, m_max, d, sw) == launches and name in launches, what
    mem = ic.members(case)
    assert len(mem["m"]) == B and mem["A"].shape == (B, m_max, d)
    before = {k: os.environ.get(k) for k in sw}
    with switches(sw):
        got = run(pa, call, mem)
        if B > ic.LARGE_B:
            ref = chunked_on_16_lanes(pa, plans, case, mem)
    assert {k: os.environ.get(k) for k in sw} == before
    if call == "pairs":
        pairs_vs_oracle(oracle, got, mem, what)
        return
    if B > ic.LARGE_B:
        free = np.flatnonzero(mem["fam"] == "unbounded")
        if call == "reduce":
            assert _same(got, ref), what
            assert _same_bits({k: v[free] for k, v in got.items()}, {k: v[free] for k, v in ref.items()}), what
        else:
            assert np.array_equal(got["status"], ref["status"]), what
            for k in ("lb", "ub"):
                assert np.allclose(got[k], ref[k], rtol=0.0, atol=1e-9, equal_nan=True), (what, k)
                assert np.array_equal(got[k][free].view(np.uint8), ref[k][free].view(np.uint8)), (what, k)
    VS_ORACLE[call](oracle, got, mem, ic.oracle_members(case), what)


def test_lp_counts_rarely_differ():
    """Over the reduce cases above: the members whose LP count differs from the oracle's with a row on the prefilter's
    threshold (the only difference the rule allows) stay below one in a thousand."""
    assert LP_COUNTS["differ"] * 1000 <= LP_COUNTS["members"], LP_COUNTS
