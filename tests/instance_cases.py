"""Which template instances of the fused reduce() and of the stand-alone LP, Chebyshev, box and pair batches the dispatch can
launch, and the smallest call that launches each -- computed from the two plan headers (polytope_amd/csrc/plp_reduce_plan.hpp,
plp_lp_plan.hpp) through the compiled plan libraries of tests/test_reduce_plan.py and tests/test_lp_plan.py (their `plan`
fixtures; every function below that asks a plan takes the two as `plans = {"reduce": ..., "lp": ...}`).

census(plans)            the plans asked over the whole size envelope and every set of up to three A/B switches: per call every
                         kernel name a plan returns, whether no switch is needed for it, and the smallest case that launches it
reachable / default_reachable   the names alone
CASES                    the table of those cases as profiles/kernel_instances.json records it (a committed file, so that the
                         GPU module can be parametrised without a compiler; tests/test_kernel_instances_host.py holds it equal
                         to census()): (call, B, m_max, d, switches, instance, launches)
members(case)            the batch of a case: the seven families of scripts/soak_lane.py: make, padded with random members

Sizes: d (LPs: n) over the envelope; row counts on both sides of every tile shape's capacity; B = 1, the smallest batch a
case can have, and both sides of every threshold the plan hosts export (tests/cabi/*_plan_host.cpp: *_plan_thresholds -- a
new threshold macro is added there and moves the census with it).  Batches beyond the grid limit of 2^31 are left to the
plan tables."""
import ctypes as C
import itertools
import json
import os
import re
import sys
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, "tests"), os.path.join(ROOT, "scripts")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import test_lp_plan as LPP  # noqa: E402
import test_reduce_plan as RP  # noqa: E402

CENSUS_FILE = os.path.join(ROOT, "profiles", "kernel_instances.json")
TRACE_FILE = os.path.join(ROOT, "profiles", "kernel_instances_trace.json")
CALLS = ("reduce", "lp", "cheby", "bbox", "pairs")
FAMILIES = ("random", "ragged", "unbounded", "dup", "scaled", "flat", "lattice")
# members per family: 16; the pair calls 4 (28 cells are 378 pairs, each against two LPs of the oracle)
PER_FAMILY = {"reduce": 16, "lp": 16, "cheby": 16, "bbox": 16, "pairs": 4}
LARGE_B = 2000      # cases beyond: the lane engines' large tile shapes; every 37th member against the oracle
ORACLE_STRIDE = 37

ROWS = (1, 8, 9, 16, 17, 32, 33, 64)
# (d or n, row counts) per call; 65 rows: the LDS engines of the LP and Chebyshev batches; pairs: the stacked pair has 2 m_max rows
SIZES = {
    "reduce": (range(1, 17), ROWS),
    "lp": (range(1, 18), ROWS + (65,)),
    "cheby": (range(1, 17), ROWS + (65,)),
    "bbox": (range(1, 17), ROWS),
    "pairs": (range(1, 17), (1, 8, 9, 16, 17, 32)),
}
# the switches a call's plan reads, with the values that mean something to it
SWITCHES = {
    "reduce": {"LANE": "01", "LANE_GS": ("4", "8", "16"), "LANE_MIX": ("0", "24"), "RETRY_ALL": "1", "1ROW": "1", "R1": "01",
               "R2": "0", "LAZY": "01", "SPLIT": "01", "HALF": "01", "WSPLIT": "024", "WDENSE": "01"},
    "lp": {"LDS": "1", "LP_WIDE": "01", "LP_1ROW": "1"},
    "cheby": {"LDS": "1", "CHEBY_WIDE": "01", "CHEBY_1ROW": "1", "CHEBY_RETRY_ALL": "1"},
    "bbox": {"CHEBY_RETRY_ALL": "1", "BBOX_LANE": "0", "BBOX_SPLIT": "01", "BBOX_WIDE": "01", "BBOX_WSPLIT": "01",
             "BBOX_WSPLIT_MAXB": ("0",), "BBOX_WDENSE": "01"},
    "pairs": {"CHEBY_RETRY_ALL": "1", "ADJ_WIDE": "01"},
}
MAX_SWITCHES = 3


def prefix(call):
    return "PLP_REDUCE_" if call == "reduce" else "PLP_"


def min_members(call):
    return len(FAMILIES) * PER_FAMILY[call]


def switch_sets(call):
    """{} first, then every choice of up to MAX_SWITCHES switches with every combination of their values."""
    sw = SWITCHES[call]
    for n in range(MAX_SWITCHES + 1):
        for keys in itertools.combinations(sorted(sw), n):
            for vals in itertools.product(*[tuple(sw[k]) for k in keys]):
                yield dict(zip(keys, vals))


def batch_sizes(plans, call):
    """1, the smallest batch of a case, and t, t + 1 for every threshold t of the call's plan."""
    buf = (C.c_longlong * 256)()
    if call == "reduce":
        n = plans["reduce"].lib.reduce_plan_thresholds(buf, 256)
    else:
        n = plans["lp"].lib.lp_plan_thresholds(LPP.CALLS.index(call), buf, 256)
    assert 0 <= n < 256
    return sorted({1, min_members(call)} | {t + k for t in buf[:n] for k in (0, 1) if t + k >= 1})


def sweep(plans, call, env):
    """Every launch the plan of `call` returns under `env` over SIZES x batch_sizes: int64[n, 9] of
    d, m_max, B, position in the call, engine, gs, rows, nw, dense."""
    ds, ms = (np.asarray(list(v), np.int32) for v in SIZES[call])
    Bs = np.asarray(batch_sizes(plans, call), np.int64)
    keys = RP.KEYS if call == "reduce" else LPP.KEYS
    assert set(env) <= set(keys)
    arr = (C.c_char_p * len(keys))(*[(env[k].encode() if k in env else None) for k in keys])
    out = np.zeros((3 * len(ds) * len(ms) * len(Bs), 9), np.int64)
    ptr = lambda a, t: a.ctypes.data_as(C.POINTER(t))  # noqa: E731
    args = (arr, ptr(ds, C.c_int), len(ds), ptr(ms, C.c_int), len(ms), ptr(Bs, C.c_longlong), len(Bs), ptr(out, C.c_longlong))
    if call == "reduce":
        fn = plans["reduce"].lib.reduce_plan_sweep
        fn.restype = C.c_longlong
        n = fn(*args)
    else:
        fn = plans["lp"].lib.lp_plan_sweep
        fn.restype = C.c_longlong
        n = fn(LPP.CALLS.index(call), *args)
    return out[:n]


def name_of(call, rec):
    d, _m, _B, pos, engine, gs, rows, nw, dense = (int(v) for v in rec)
    if call == "reduce":
        return RP.kernel_name(d, dict(engine=RP.ENGINES[engine], gs=gs, rows=rows, nw=nw, dense=dense))
    return LPP.kernel_name(call, d, dict(engine=LPP.ENGINES[engine], gs=gs, rows=rows, nw=nw, dense=dense), pos)


def natural(name):
    return [int(t) if t.isdigit() else t for t in re.split(r"(\d+)", name)]


def planned(plans, call, B, m_max, d, switches):
    """The kernel names of one call in launch order (None: the size is refused).  switches: as the environment spells them."""
    env = {k[len(prefix(call)):]: str(v) for k, v in switches.items()}
    if call == "reduce":
        return RP.planned_kernels(plans["reduce"], B, m_max, d, env)
    sizes = (B, m_max, d) + ((0, 0, 0, 0) if call == "pairs" else ())
    rows, _ = LPP.planned(plans["lp"], call, sizes, env)
    return None if rows is None else [r[0] for r in rows]


_CENSUS = {}


def census_of(plans, call):
    """-> {kernel name: dict(default=..., case=dict(B, m_max, d, switches, launches))}.  The case of an instance: among the
    calls of at least min_members(call) members that launch it, first those that launch it FIRST (the phase-1 and retry
    kernels of the generic LPs never are), then the smallest batch, the fewest switches, the most rows."""
    memo = (id(plans["reduce"]), id(plans["lp"]), call)   # (the plans are compiled once per test module)
    if memo in _CENSUS:
        return _CENSUS[memo]
    best, default = {}, set()
    for env in switch_sets(call):
        R = sweep(plans, call, env)
        if not len(R):
            continue
        inst = R[:, [0, 3, 4, 5, 6, 7, 8]]
        # per instance the record with the best key: runnable (B >= the smallest batch) before not, first launch, B, rows
        small = (R[:, 2] < min_members(call)).astype(np.int64)
        order = np.lexsort((-R[:, 1], R[:, 2], R[:, 3] > 0, small) + tuple(inst.T[::-1]))
        S, I = R[order], inst[order]
        firsts = np.flatnonzero(np.r_[True, np.any(I[1:] != I[:-1], axis=1)])
        for i in firsts:
            name = name_of(call, S[i])
            if not env:
                default.add(name)
            key = (int(S[i, 2] < min_members(call)), int(S[i, 3] > 0), int(S[i, 2]), len(env), -int(S[i, 1]), sorted(env.items()))
            if name not in best or key < best[name][0]:
                best[name] = (key, (int(S[i, 2]), int(S[i, 1]), int(S[i, 0]), dict(env)))
    out = {}
    for name in sorted(best, key=natural):
        key, (B, m_max, d, env) = best[name]
        assert key[0] == 0, "%s is launched only by batches of fewer than %d members" % (name, min_members(call))
        sw = {prefix(call) + k: v for k, v in sorted(env.items())}
        launches = planned(plans, call, B, m_max, d, sw)
        assert name in launches, (name, launches)
        out[name] = dict(default=name in default, case=dict(B=B, m_max=m_max, d=d, switches=sw, launches=launches))
    _CENSUS[memo] = out
    return out


def launchable_reduce():
    """The instances plp_reduce_launch.hpp names: the templates its switch over (engine, gs, rows, nw) can launch per D."""
    names = set()
    for d in range(1, 17):
        names.add("reduce_kernel<%d>" % d)
        if d <= 4:
            names |= {"reduce_lane_kernel<%d, %d, %d>" % (d, gs, rows) for gs, rows in ((16, 32), (8, 32), (16, 16), (8, 16), (4, 16))}
            names |= {"reduce_lane_mix_kernel<%d, 32, 8, 16>" % d, "reduce_lane_mix_kernel<%d, 16, 4, 8>" % d}
            names.add("reduce_r_mix_kernel<%d>" % d)
        if d <= 8:
            shapes = [(gs, 4) for gs in (4, 8, 16)] + ([(gs, 2) for gs in (8, 16, 32)] if d >= 5 else [])
            split = [(gs, 4) for gs in (4, 8, 16)]
        else:
            shapes, split = [(64, 1), (16, 2), (32, 2)], [(16, 2), (32, 2)]
        names |= {"reduce_r_kernel<%d, %d, %d>" % ((d,) + s) for s in shapes}
        names |= {"reduce_split_kernel<%d, %d, %d>" % ((d,) + s) for s in split}
        if d >= 5:
            t = "true" if d <= 13 else "false"
            names |= {"reduce_wdense_kernel<%d>" % d, "reduce_lazy_kernel<%d>" % d,
                      "reduce_wsplit_kernel<%d, 4, %s>" % (d, t), "reduce_wsplit_kernel<%d, 2, %s>" % (d, t)}
    return names


def census(plans):
    """What profiles/kernel_instances.json holds."""
    out = {"calls": {}}
    for call in CALLS:
        got = census_of(plans, call)
        out["calls"][call] = {"instances": [dict(name=n, **v) for n, v in got.items()]}
    named = launchable_reduce()
    reached = {i["name"] for i in out["calls"]["reduce"]["instances"]}
    assert reached <= named, sorted(reached - named)
    out["calls"]["reduce"]["unreachable"] = sorted(named - reached, key=natural)
    return out


def reachable(plans, call):
    return set(census_of(plans, call))


def default_reachable(plans, call):
    return {n for n, v in census_of(plans, call).items() if v["default"]}


def write_census(plans, path=CENSUS_FILE):
    with open(path, "w") as f:
        json.dump(census(plans), f, indent=1, sort_keys=True)
        f.write("\n")


def load_cases(path=CENSUS_FILE):
    with open(path) as f:
        rec = json.load(f)
    rows = []
    for call in CALLS:
        for inst in rec["calls"][call]["instances"]:
            c = inst["case"]
            rows.append((call, c["B"], c["m_max"], c["d"], c["switches"], inst["name"], c["launches"]))
    return rows


# (call, B, m_max, d, switches as the environment spells them, the instance the case is for, every kernel of the call in order)
CASES = load_cases() if os.path.exists(CENSUS_FILE) else []


def case_id(case):
    call, B, m_max, d, switches, name, _ = case
    sw = ",".join("%s=%s" % (k[len(prefix(call)):], v) for k, v in sorted(switches.items())) or "default"
    return "%s-%s-B%d-m%d-%s" % (call, name.replace(" ", ""), B, m_max, sw)


# The seed of a case is the CRC of its id, plus what stands here: the reduce cases whose first draw put a row of a bounded
# member on the threshold of reduce()'s prefilter (family `dup` where a copied row replaces a side of the box and the
# polytope reaches 1e2 .. 1e7: scripts/soak_lane.py: prefilter_tie measures the threshold against that extent) took the next
# seed without one.  tests/test_kernel_instances_host.py: test_inputs_rarely_tie_at_the_prefilter holds the condition.
RESEEDED = {
    'reduce-reduce_r_kernel<11,16,2>-B112-m32-LAZY=0,SPLIT=0': 10,
    'reduce-reduce_r_kernel<12,16,2>-B112-m32-LAZY=0,SPLIT=0': 27,
    'reduce-reduce_r_kernel<13,16,2>-B112-m32-LAZY=0,SPLIT=0': 53,
    'reduce-reduce_r_kernel<14,16,2>-B112-m32-LAZY=0,SPLIT=0': 16,
    'reduce-reduce_r_kernel<15,16,2>-B112-m32-LAZY=0,SPLIT=0': 4,
    'reduce-reduce_r_kernel<16,16,2>-B112-m32-LAZY=0,SPLIT=0': 16,
    'reduce-reduce_r_kernel<4,4,4>-B112-m16-HALF=0,SPLIT=0': 1,
    'reduce-reduce_r_kernel<5,8,2>-B112-m16-SPLIT=0': 1,
    'reduce-reduce_r_kernel<6,8,2>-B112-m16-SPLIT=0': 2,
    'reduce-reduce_r_kernel<7,8,2>-B112-m16-SPLIT=0': 6,
    'reduce-reduce_r_kernel<8,8,2>-B112-m16-SPLIT=0': 3,
    'reduce-reduce_r_mix_kernel<4>-B112-m16-SPLIT=0': 1,
    'reduce-reduce_split_kernel<10,16,2>-B112-m32-LAZY=0': 2,
    'reduce-reduce_split_kernel<11,16,2>-B112-m32-LAZY=0': 2,
    'reduce-reduce_split_kernel<12,16,2>-B112-m32-LAZY=0': 84,
    'reduce-reduce_split_kernel<13,16,2>-B112-m32-LAZY=0': 35,
    'reduce-reduce_split_kernel<14,16,2>-B112-m32-LAZY=0': 4,
    'reduce-reduce_split_kernel<15,16,2>-B112-m32-LAZY=0': 8,
    'reduce-reduce_split_kernel<16,16,2>-B112-m32-LAZY=0': 2,
    'reduce-reduce_split_kernel<5,4,4>-B112-m16-HALF=0': 1,
    'reduce-reduce_split_kernel<6,4,4>-B112-m16-HALF=0': 2,
    'reduce-reduce_split_kernel<7,4,4>-B112-m16-HALF=0': 6,
    'reduce-reduce_split_kernel<8,4,4>-B112-m16-HALF=0': 1,
}


def members(case):
    """The batch of a case -> dict(fam: family name per member, A, b, m; lp: also c).  Seven families of 16 (pairs: 4)
    members from scripts/soak_lane.py: make, m[p] ragged as make returns it, then `random` members up to B.
    lp: random costs, and every other member's feasible set moved off the origin (phase 1 runs), as scripts/soak_lp.py does.
    pairs: every cell moved by a random vector, so that cells overlap, touch nothing and lie apart."""
    import soak_lane as SL
    call, B, m_max, d = case[:4]
    rng = np.random.default_rng(zlib.crc32(case_id(case).encode()) + RESEEDED.get(case_id(case), 0))
    per = PER_FAMILY[call]
    assert B >= per * len(FAMILIES)
    parts = [(fam, SL.make(rng, per, m_max, d, fam)) for fam in FAMILIES]
    if B > per * len(FAMILIES):
        parts.append(("random", SL.make(rng, B - per * len(FAMILIES), m_max, d, "random")))
    out = dict(fam=np.concatenate([[fam] * len(p[2]) for fam, p in parts]), A=np.concatenate([p[0] for _, p in parts]),
               b=np.concatenate([p[1] for _, p in parts]), m=np.concatenate([p[2] for _, p in parts]).astype(np.int32))
    if call == "lp":
        shift = rng.standard_normal((B, d)) * 2.0
        shift[0::2] = 0.0
        out["b"] = out["b"] + np.einsum("bij,bj->bi", out["A"], shift)
        out["c"] = rng.standard_normal((B, d))
    if call == "pairs":
        out["b"] = out["b"] + np.einsum("bij,bj->bi", out["A"], rng.uniform(-1.0, 1.0, (B, d)))
    return out


def oracle_members(case):
    """The members of a case that go against the oracle: all of them, every 37th of a large case."""
    return range(0, case[1], ORACLE_STRIDE if case[1] > LARGE_B else 1)
