"""CPU: the fused reduce's plan (polytope_amd/csrc/plp_reduce_plan.hpp) -- which kernel runs a batch (B, m_max, d) under
which A/B switches, with what tile shape, grid, workgroup and LDS, and whether the general kernel's second pass follows.
The header is pure host code; it is compiled here with g++ and called through ctypes (tests/cabi/reduce_plan_host.cpp).
The table straddles every threshold of the header and covers each switch the GPU tests use; its values are the launches
the dispatch made before it was gathered into the plan, checked against a kernel trace on the device."""
import ctypes as C
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("LANE", "LANE_GS", "LANE_MIX", "RETRY_ALL", "1ROW", "R1", "R2", "LAZY", "SPLIT", "HALF", "WSPLIT", "WDENSE")
ENGINES = ("NONE", "GENERAL", "LANE", "LANE_MIX", "GROUP", "GROUP_MIX", "SPLIT", "WDENSE", "LAZY", "WSPLIT")
FIELDS = ("engine", "gs", "rows", "nw", "dense", "nbig", "grid", "block", "lds", "second", "force_retry",
          "retry_gs", "retry_grid", "retry_lds")

# (B, m_max, d, {switch: value}) -> (engine, gs, rows, nw, dense, nbig, grid, block, lds, second, force_retry,
#                                    gs / grid / LDS of the second pass)
CASES = [
    ((100000, 16, 3, {}), ('LANE_MIX', 4, 16, 0, 0, 5469, 7031, 64, 10240, 0, 0, 16, 2048, 8192)),
    ((1, 16, 3, {}), ('LANE', 16, 16, 0, 0, 0, 1, 64, 2560, 0, 0, 16, 1, 8192)),
    ((14000, 16, 3, {}), ('LANE', 16, 16, 0, 0, 0, 3500, 64, 2560, 0, 0, 16, 875, 8192)),
    ((14001, 16, 3, {}), ('LANE', 8, 16, 0, 0, 0, 1751, 64, 5120, 0, 0, 16, 876, 8192)),
    ((40000, 16, 3, {}), ('LANE', 8, 16, 0, 0, 0, 5000, 64, 5120, 0, 0, 16, 2048, 8192)),
    ((40001, 16, 3, {}), ('LANE_MIX', 4, 16, 0, 0, 2189, 2812, 64, 10240, 0, 0, 16, 2048, 8192)),
    ((16384, 16, 3, {}), ('LANE', 8, 16, 0, 0, 0, 2048, 64, 5120, 0, 0, 16, 1024, 8192)),
    ((8193, 16, 3, {}), ('LANE', 16, 16, 0, 0, 0, 2049, 64, 2560, 0, 0, 16, 513, 8192)),
    ((100000, 16, 3, {'LANE_GS': '4'}), ('LANE', 4, 16, 0, 0, 0, 6250, 64, 10240, 0, 0, 16, 2048, 8192)),
    ((100000, 16, 3, {'LANE_MIX': '0'}), ('LANE', 4, 16, 0, 0, 0, 6250, 64, 10240, 0, 0, 16, 2048, 8192)),
    ((100000, 16, 3, {'LANE_MIX': '8'}), ('LANE_MIX', 4, 16, 0, 0, 5469, 7031, 64, 10240, 0, 0, 16, 2048, 8192)),
    ((16000, 24, 3, {}), ('LANE', 16, 32, 0, 0, 0, 4000, 64, 5120, 0, 0, 32, 2000, 8192)),
    ((16001, 24, 3, {}), ('LANE_MIX', 8, 32, 0, 0, 1751, 2250, 64, 10240, 0, 0, 32, 2001, 8192)),
    ((16001, 24, 4, {}), ('LANE', 8, 32, 0, 0, 0, 2001, 64, 12288, 0, 0, 32, 2001, 10240)),
    ((16001, 24, 3, {'LANE_GS': '16'}), ('LANE', 16, 32, 0, 0, 0, 4001, 64, 5120, 0, 0, 32, 2001, 8192)),
    ((40000, 12, 4, {}), ('GROUP', 4, 4, 0, 0, 0, 2500, 64, 12288, 1, 0, 16, 2048, 10240)),
    ((40001, 12, 4, {}), ('LANE_MIX', 4, 16, 0, 0, 2189, 2812, 64, 12288, 0, 0, 16, 2048, 10240)),
    ((3000, 14, 4, {}), ('SPLIT', 4, 4, 0, 0, 0, 3000, 64, 848, 1, 0, 16, 188, 10240)),
    ((3001, 14, 4, {}), ('LANE', 16, 16, 0, 0, 0, 751, 64, 3072, 0, 0, 16, 188, 10240)),
    ((40000, 12, 4, {'HALF': '1'}), ('GROUP_MIX', 4, 4, 0, 0, 0, 5000, 64, 12288, 1, 0, 16, 2048, 10240)),
    ((100000, 16, 3, {'LANE': '0'}), ('GROUP_MIX', 4, 4, 0, 0, 6055, 6445, 64, 10240, 1, 0, 16, 2048, 8192)),
    ((100000, 16, 3, {'SPLIT': '0'}), ('GROUP_MIX', 4, 4, 0, 0, 6055, 6445, 64, 10240, 1, 0, 16, 2048, 8192)),
    ((100000, 16, 3, {'SPLIT': '1'}), ('SPLIT', 4, 4, 0, 0, 0, 100000, 64, 704, 1, 0, 16, 2048, 8192)),
    ((20000, 16, 3, {'HALF': '0'}), ('GROUP', 4, 4, 0, 0, 0, 1250, 64, 10240, 1, 0, 16, 1250, 8192)),
    ((4096, 16, 3, {'LANE': '0'}), ('SPLIT', 4, 4, 0, 0, 0, 4096, 64, 704, 1, 0, 16, 256, 8192)),
    ((4097, 16, 3, {'LANE': '0'}), ('GROUP_MIX', 4, 4, 0, 0, 0, 513, 64, 10240, 1, 0, 16, 257, 8192)),
    ((500, 48, 2, {'LANE': '1'}), ('SPLIT', 16, 4, 0, 0, 0, 500, 64, 2096, 1, 0, 64, 125, 6144)),
    ((1500, 16, 6, {}), ('WSPLIT', 64, 1, 4, 1, 0, 1500, 256, 6336, 0, 0, 16, 94, 14336)),
    ((1501, 16, 6, {}), ('SPLIT', 4, 4, 0, 0, 0, 1501, 64, 1136, 1, 0, 16, 94, 14336)),
    ((2049, 16, 6, {}), ('GROUP', 8, 2, 0, 0, 0, 257, 64, 8192, 1, 0, 16, 129, 14336)),
    ((20000, 24, 6, {}), ('GROUP', 16, 2, 0, 0, 0, 5000, 64, 8192, 1, 0, 32, 2048, 14336)),
    ((20000, 48, 6, {}), ('WDENSE', 64, 1, 0, 0, 0, 20000, 64, 4352, 0, 0, 64, 2048, 14336)),
    ((12000, 48, 8, {}), ('WSPLIT', 64, 1, 4, 1, 0, 12000, 256, 7600, 0, 0, 64, 2048, 18432)),
    ((12001, 48, 8, {}), ('WSPLIT', 64, 1, 2, 1, 0, 12001, 128, 6640, 0, 0, 64, 2048, 18432)),
    ((16001, 48, 8, {}), ('WDENSE', 64, 1, 0, 0, 0, 16001, 64, 5376, 0, 0, 64, 2048, 18432)),
    ((1501, 16, 7, {}), ('GROUP', 8, 2, 0, 0, 0, 188, 64, 9216, 1, 0, 16, 94, 16384)),
    ((1000, 16, 6, {'SPLIT': '0'}), ('GROUP', 8, 2, 0, 0, 0, 125, 64, 8192, 1, 0, 16, 63, 14336)),
    ((500, 48, 6, {'LAZY': '0'}), ('SPLIT', 16, 4, 0, 0, 0, 500, 64, 4208, 1, 0, 64, 125, 14336)),
    ((50000, 16, 6, {'LAZY': '1'}), ('WDENSE', 64, 1, 0, 0, 0, 50000, 64, 4352, 0, 0, 16, 2048, 14336)),
    ((1000, 48, 6, {'WDENSE': '0'}), ('LAZY', 64, 1, 0, 0, 0, 1000, 64, 4352, 1, 0, 64, 250, 14336)),
    ((1000, 48, 14, {'WDENSE': '1'}), ('WDENSE', 64, 1, 0, 0, 0, 1000, 64, 8704, 0, 0, 64, 250, 30720)),
    ((1000, 48, 6, {'WSPLIT': '0'}), ('WDENSE', 64, 1, 0, 0, 0, 1000, 64, 4352, 0, 0, 64, 250, 14336)),
    ((1000, 48, 6, {'WSPLIT': '2'}), ('WSPLIT', 64, 1, 2, 1, 0, 1000, 128, 5472, 0, 0, 64, 250, 14336)),
    ((50000, 48, 9, {'WSPLIT': '4'}), ('WSPLIT', 64, 1, 4, 1, 0, 50000, 256, 8200, 0, 0, 64, 2048, 20480)),
    ((1500, 32, 10, {}), ('WSPLIT', 64, 1, 4, 1, 0, 1500, 256, 8800, 0, 0, 32, 188, 22528)),
    ((1501, 32, 10, {}), ('GROUP', 16, 2, 0, 0, 0, 376, 64, 12288, 1, 0, 32, 188, 22528)),
    ((2001, 32, 13, {}), ('GROUP', 16, 2, 0, 0, 0, 501, 64, 15360, 1, 0, 32, 251, 28672)),
    ((3000, 48, 14, {}), ('WSPLIT', 64, 1, 2, 0, 0, 3000, 128, 10080, 1, 0, 64, 750, 30720)),
    ((3001, 48, 14, {}), ('LAZY', 64, 1, 0, 0, 0, 3001, 64, 8704, 1, 0, 64, 751, 30720)),
    ((20000, 64, 16, {}), ('LAZY', 64, 1, 0, 0, 0, 20000, 64, 9728, 1, 0, 64, 2048, 34816)),
    ((5000, 48, 10, {'R1': '1'}), ('GROUP', 64, 1, 0, 0, 0, 5000, 64, 6144, 1, 0, 64, 1250, 22528)),
    ((1000, 16, 10, {'R1': '0'}), ('SPLIT', 16, 2, 0, 0, 0, 1000, 64, 3248, 1, 0, 16, 63, 22528)),
    ((1000, 16, 10, {'R2': '0'}), ('GENERAL', 16, 1, 0, 0, 0, 63, 256, 22528, 0, 0, 16, 63, 22528)),
    ((100000, 16, 3, {'1ROW': '1'}), ('GENERAL', 16, 1, 0, 0, 0, 6250, 256, 8192, 0, 0, 16, 2048, 8192)),
    ((100000, 16, 3, {'RETRY_ALL': '1'}), ('LANE_MIX', 4, 16, 0, 0, 5469, 7031, 64, 10240, 0, 1, 16, 2048, 8192)),
    ((1500, 16, 6, {'RETRY_ALL': '1'}), ('WSPLIT', 64, 1, 4, 1, 0, 1500, 256, 6336, 1, 1, 16, 94, 14336)),
    ((10, 0, 3, {}), ('GENERAL', 8, 1, 0, 0, 0, 1, 256, 8192, 0, 0, 8, 1, 8192)),
    ((10, 65, 3, {}), ('NONE', 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0)),
    ((10, 16, 17, {}), ('NONE', 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0)),
]


def kernel_name(d, L):
    """The kernel a planned launch stands for, as a trace names it (the templates of plp_reduce_launch.hpp).  L: a dict with
    engine (its name), gs, rows, nw."""
    e = L["engine"]
    if e == "GENERAL":
        return "reduce_kernel<%d>" % d
    if e == "LANE":
        return "reduce_lane_kernel<%d, %d, %d>" % (d, L["gs"], L["rows"])
    if e == "LANE_MIX":
        return "reduce_lane_mix_kernel<%d, %d, %d, %d>" % (d, L["rows"], L["gs"], 2 * L["gs"])
    if e in ("GROUP", "SPLIT"):
        return "reduce_%s_kernel<%d, %d, %d>" % ("r" if e == "GROUP" else "split", d, L["gs"], L["rows"])
    if e == "WSPLIT":   # (with the dense LPs up to PLP_REDUCE_WDENSE_MAXD and without beyond: the plan's `dense` says which)
        return "reduce_wsplit_kernel<%d, %d, %s>" % (d, L["nw"], "true" if L["dense"] else "false")
    return {"GROUP_MIX": "reduce_r_mix_kernel<%d>", "WDENSE": "reduce_wdense_kernel<%d>", "LAZY": "reduce_lazy_kernel<%d>"}[e] % d


def planned_kernels(plan, B, m, d, env):
    """The kernels of a call in launch order: the first launch, then reduce_kernel<D> where the second pass follows."""
    got = dict(zip(FIELDS, plan(B, m, d, env)))
    if got["engine"] == "NONE":
        return None
    return [kernel_name(d, got)] + (["reduce_kernel<%d>" % d] if got["second"] else [])


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("plan") / "libreduce_plan.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-fPIC", "-shared", "-o", out,
                           os.path.join(ROOT, "tests", "cabi", "reduce_plan_host.cpp")])
    L = C.CDLL(out)
    L.reduce_plan.argtypes = [C.c_longlong, C.c_int, C.c_int, C.POINTER(C.c_char_p), C.POINTER(C.c_longlong)]
    L.reduce_plan.restype = None

    def run(B, m, d, env):
        assert set(env) <= set(KEYS)
        arr = (C.c_char_p * len(KEYS))(*[(env[k].encode() if k in env else None) for k in KEYS])
        o = (C.c_longlong * len(FIELDS))()
        L.reduce_plan(B, m, d, arr, o)
        return (ENGINES[o[0]],) + tuple(o[1:])
    run.lib = L   # (reduce_plan_thresholds, reduce_plan_sweep: tests/instance_cases.py)
    return run


def test_kernel_names(plan):
    assert planned_kernels(plan, 100000, 16, 3, {}) == ["reduce_lane_mix_kernel<3, 16, 4, 8>"]
    assert planned_kernels(plan, 16001, 24, 3, {}) == ["reduce_lane_mix_kernel<3, 32, 8, 16>"]
    assert planned_kernels(plan, 300, 32, 12, {"LAZY": "0", "SPLIT": "0"}) == ["reduce_r_kernel<12, 16, 2>", "reduce_kernel<12>"]
    assert planned_kernels(plan, 300, 32, 9, {"LAZY": "1", "WSPLIT": "0"}) == ["reduce_wdense_kernel<9>"]
    assert planned_kernels(plan, 3000, 48, 14, {}) == ["reduce_wsplit_kernel<14, 2, false>", "reduce_kernel<14>"]
    assert planned_kernels(plan, 1000, 16, 9, {"WSPLIT": "2"}) == ["reduce_wsplit_kernel<9, 2, true>"]
    assert planned_kernels(plan, 10, 65, 3, {}) is None


@pytest.mark.parametrize("case,want", CASES, ids=["%d-%d-%d-%s" % (c[0][0], c[0][1], c[0][2], ",".join(
    "%s=%s" % kv for kv in sorted(c[0][3].items())) or "default") for c in CASES])
def test_plan_table(plan, case, want):
    got = plan(*case)
    assert got == want, {f: (g, w) for f, g, w in zip(FIELDS, got, want) if g != w}


def test_bench_shape(plan):
    """the benchmark: (16,3) x 100 000 on reduce_lane_mix_kernel<3,16,4,8>, 5 469 tiles of 16 polytopes and 1 562 of 8,
    workgroups of one wavefront, complete in one launch"""
    got = dict(zip(FIELDS, plan(100000, 16, 3, {})))
    assert got["engine"] == "LANE_MIX" and (got["gs"], got["rows"]) == (4, 16)
    assert got["nbig"] == 5469 and got["grid"] == 5469 + 1562 and got["block"] == 64
    assert got["second"] == 0


def test_switch_presence(plan):
    """a lane-group switch keeps the lane-group forms whatever its value; an empty value counts as set"""
    assert plan(100000, 16, 3, {"HALF": ""})[0] == "GROUP_MIX"
    assert plan(100000, 16, 3, {"SPLIT": "x"})[0] == "GROUP_MIX"
    assert plan(1000, 16, 6, {"HALF": "0"})[0] == "SPLIT"
