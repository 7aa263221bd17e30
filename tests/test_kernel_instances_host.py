"""CPU: the census of kernel instances (tests/instance_cases.py) -- every instance a plan can return has a case in the table
that launches it, the committed profiles/kernel_instances.json is the computed census, the recorded device trace (when
present) names the kernels the table names, and the inputs of tests/test_kernel_instances_gpu.py rarely sit on the
threshold of reduce()'s prefilter.

PLP_WRITE_CENSUS=1 pytest tests/test_kernel_instances_host.py -k census   rewrites the committed file from the plans."""
import json
import os

import pytest

import instance_cases as ic
from test_lp_plan import plan as lp_plan  # noqa: F401 (a fixture: the compiled plan)
from test_reduce_plan import plan as reduce_plan  # noqa: F401 (likewise)


@pytest.fixture(scope="module")
def plans(reduce_plan, lp_plan):  # noqa: F811
    return {"reduce": reduce_plan, "lp": lp_plan}


@pytest.fixture(scope="module")
def computed(plans):
    if os.environ.get("PLP_WRITE_CENSUS") == "1":
        ic.write_census(plans)
    return ic.census(plans)


def test_census_file_is_the_computed_census(computed):
    with open(ic.CENSUS_FILE) as f:
        assert json.load(f) == computed
    assert ic.CASES == ic.load_cases()


@pytest.mark.parametrize("call", ic.CALLS)
def test_every_reachable_instance_has_a_case(plans, computed, call):
    """Every name the plan of `call` can return is the instance of one row of CASES, and every row's planned launches are
    what the row says.  A new instance in a plan fails here until the census file has a case for it."""
    rows = [c for c in ic.CASES if c[0] == call]
    want = ic.reachable(plans, call)
    assert {c[5] for c in rows} == want, (sorted(want - {c[5] for c in rows}), sorted({c[5] for c in rows} - want))
    assert len(rows) == len(want)
    for c in rows:
        _, B, m_max, d, switches, name, launches = c
        assert B >= ic.min_members(call) and len(switches) <= ic.MAX_SWITCHES, c
        assert ic.planned(plans, call, B, m_max, d, switches) == launches and name in launches, c
        if B > ic.LARGE_B:   # the large cases are the lane engines' tile shapes: the GPU module's chunk rule is theirs
            assert name.startswith(("reduce_lane_kernel", "reduce_lane_mix_kernel", "bbox_lane_kernel")), c
    flagged = {i["name"] for i in computed["calls"][call]["instances"] if i["default"]}
    assert flagged == ic.default_reachable(plans, call) and flagged <= want


def test_counts(computed):
    """The size of the space (the figures of DESIGN.md 6b): a change of the plans that adds or loses instances shows here."""
    n = {call: (len(v["instances"]), sum(i["default"] for i in v["instances"])) for call, v in computed["calls"].items()}
    assert n == {"reduce": (183, 106), "lp": (96, 40), "cheby": (85, 57), "bbox": (111, 67), "pairs": (36, 32)}, n
    un = computed["calls"]["reduce"]["unreachable"]
    assert len(un) == 13 and len(ic.launchable_reduce()) == 196, un


def test_case_ids_are_unique():
    ids = [ic.case_id(c) for c in ic.CASES]
    assert len(set(ids)) == len(ids)
    assert set(ic.RESEEDED) <= set(ids), sorted(set(ic.RESEEDED) - set(ids))


def test_trace_agrees_with_the_table():
    """profiles/kernel_instances_trace.json (scripts/trace_lp_plan.py --instances, a kernel trace of the table on the device):
    per case the kernels traced are the kernels of the table, in order."""
    if not os.path.exists(ic.TRACE_FILE):
        pytest.skip("no recorded trace")
    with open(ic.TRACE_FILE) as f:
        traced = json.load(f)["cases"]
    table = {ic.case_id(c): c[6] for c in ic.CASES}
    assert set(traced) == set(table), sorted(set(table) ^ set(traced))[:8]
    for cid, got in traced.items():
        assert [g[0] for g in got] == table[cid], (cid, got)


def _tie_counts(case):
    """-> (members of the case that go against the oracle, those of them with a finite box and a row on the prefilter's
    threshold, those for which prefilter_tie answers True for want of a finite box)"""
    import numpy as np
    import soak_lane as SL
    from oracle import oracle as O
    mem = ic.members(case)
    n = ties = open_ = 0
    for k in ic.oracle_members(case):
        Ak, bk = mem["A"][k, :mem["m"][k]], mem["b"][k, :mem["m"][k]]
        n += 1
        if SL.prefilter_tie(Ak, bk):
            lo, hi, bad = O.bounding_box(Ak, bk)
            finite = not bad and np.all(np.isfinite(lo)) and np.all(np.isfinite(hi))
            ties, open_ = ties + int(finite), open_ + int(not finite)
    return n, ties, open_


def test_inputs_rarely_tie_at_the_prefilter(oracle):
    """The input condition of the GPU module: of the members of the reduce cases that go against the oracle, at most one in a
    thousand has a row on the threshold of reduce()'s bounding-box prefilter (scripts/soak_lane.py: prefilter_tie), where the
    LP count is decided by the last digits of the box LPs.  A property of the inputs alone (the seeds are the case ids').
    prefilter_tie also answers True for every polytope WITHOUT a finite box -- the whole family `unbounded`, every member with
    fewer than d + 1 rows -- because there it cannot evaluate the threshold; those are not ties and are not counted here (the
    prefilter does not run on them).  The GPU module bounds what that answer can excuse: LP counts that differ from the
    oracle's on at most one member in a thousand."""
    import multiprocessing as mp
    cases = [c for c in ic.CASES if c[0] == "reduce"]
    with mp.get_context("fork").Pool(max(1, min(8, os.cpu_count() or 1))) as pool:   # (the oracle is built: the fixture)
        n, ties, open_ = (sum(v) for v in zip(*pool.map(_tie_counts, cases, chunksize=4)))
    print("members %d, without a finite box %d, on the prefilter's threshold %d" % (n, open_, ties))
    assert n > 20000 and open_ < n and ties * 1000 <= n, (ties, open_, n)
