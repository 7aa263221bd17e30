"""Which kernels the stand-alone LP, Chebyshev, bounding-box and pair batches really launch, case by case of the table of
tests/test_lp_plan.py:   python scripts/trace_lp_plan.py OUT.json

Starts itself once more under `rocprofv3 --kernel-trace` (a run of its own, no counters, under a time limit).  That child
runs every case of the table with at most MAX_MEMBERS members on the device-pointer entry points of the C ABI, one after
another, with PLP_VERIFY=0 and the switches of the case in the environment, and the library's selftest kernel between them.
The trace is then cut at the selftest kernels and written as {"cases": {case id: [[kernel, workgroups, threads per workgroup,
LDS bytes], ...]}} -- kernel names as scripts/debug/trace_summary.py shortens them.  Only public entry points are used, so
the same file runs on a tree from before the plan (profiles/lp_plan_trace_before.json) and after it (..._after.json).

  python scripts/trace_lp_plan.py --instances OUT.json
The same for the table of tests/instance_cases.py (one case per kernel instance of the fused reduce and of the four calls
above, profiles/kernel_instances.json): every case's batch through the Python calls on CUDA tensors under the case's switches
-> profiles/kernel_instances_trace.json, which tests/test_kernel_instances_host.py compares with the table."""
import csv
import glob
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
MAX_MEMBERS = 50000
LIMIT_S = 420
SEPARATOR = "selftest_kernel"


INSTANCES = "--instances" in sys.argv


def runnable():
    """The cases the C ABI can pose, small enough to run (the matrix form of the pair calls has no cross pairs)."""
    if INSTANCES:
        import instance_cases as ic
        return [(ic.case_id(c), c) for c in ic.CASES]
    from test_lp_plan import CASES, case_id
    return [(case_id(c), c) for c, _ in CASES if (c[1][0] if c[0] != "pairs" else c[1][0] ** 2 // 2) <= MAX_MEMBERS
            and not (c[0] == "pairs" and c[1][6] and not c[1][5])]


def instance_worker():
    """One call per case of tests/instance_cases.py: CASES (the pair cases: the adjacency matrix), the selftest kernel between."""
    os.environ["PLP_VERIFY"] = "0"
    import numpy as np
    import torch
    import instance_cases as ic
    import polytope_amd as pa
    from polytope_amd import _lib
    lib, ctx = _lib.load(), _lib.context(0)
    sep_d, sep_u = np.zeros(128), np.zeros(128, np.uint32)
    for cid, case in runnable():
        assert lib.plp_selftest(ctx.handle, 8, sep_d.ctypes.data, sep_u.ctypes.data) == 0
        call, switches = case[0], case[4]
        mem = ic.members(case)
        A, b, m = (torch.as_tensor(np.ascontiguousarray(mem[k])).to("cuda:0") for k in ("A", "b", "m"))
        os.environ.update(switches)
        try:
            if call == "reduce":
                pa.reduce_batch(A, b, m)
            elif call == "cheby":
                pa.cheby_ball_batch(A, b, m=m)
            elif call == "bbox":
                pa.bbox_batch(A, b, m)
            elif call == "lp":
                pa.lpsolve_batch(torch.as_tensor(mem["c"]).to("cuda:0"), A, b, m)
            else:
                pa.adjacent_pairs(A, b, m)
            torch.cuda.synchronize()
        finally:
            for key in switches:
                del os.environ[key]
        print("case %s" % cid, flush=True)
    assert lib.plp_selftest(ctx.handle, 8, sep_d.ctypes.data, sep_u.ctypes.data) == 0


def worker():
    if INSTANCES:
        return instance_worker()
    os.environ["PLP_VERIFY"] = "0"
    import ctypes as C
    import numpy as np
    import torch
    from polytope_amd import _lib
    lib, ctx = _lib.load(), _lib.context(0)
    stream = C.c_void_p(torch.cuda.current_stream(0).cuda_stream)
    sep_d, sep_u = np.zeros(128), np.zeros(128, np.uint32)

    def dev(a):
        return torch.as_tensor(np.ascontiguousarray(a)).to("cuda:0")   # (a copy: no kernel of torch's in the trace)

    def out(shape, dtype):
        return torch.empty(shape, dtype=dtype, device="cuda:0")

    def ptr(t):
        return C.c_void_p(t.data_ptr())

    for k, (cid, (call, sizes, env)) in enumerate(runnable()):
        rc = lib.plp_selftest(ctx.handle, 8, sep_d.ctypes.data, sep_u.ctypes.data)
        assert rc == 0, rc
        rng = np.random.default_rng(k)
        B, m_max, d = (max(int(s), 0) for s in sizes[:3])
        rows = max(m_max, 1)   # (no NULL pointer where a table has no rows)
        A, b = dev(rng.standard_normal((B, rows, d))), dev(1.0 + rng.random((B, rows)))
        m = dev(np.full(B, m_max, np.int32))
        names = {"PLP_" + key: v for key, v in env.items()}
        os.environ.update(names)
        try:
            if call == "lp":
                c, x, fun = dev(rng.standard_normal((B, d))), out((B, d), torch.float64), out((B,), torch.float64)
                st, it = out((B,), torch.int32), out((B,), torch.int32)
                rc = lib.plp_lp_solve_batch_dev(ctx.handle, stream, sizes[0], sizes[1], sizes[2], ptr(c), ptr(A), ptr(b), ptr(m),
                                                ptr(x), ptr(fun), ptr(st), ptr(it))
            elif call == "cheby":
                r, xc, st = out((B,), torch.float64), out((B, d), torch.float64), out((B,), torch.int32)
                rc = lib.plp_cheby_batch_dev(ctx.handle, stream, sizes[0], sizes[1], sizes[2], ptr(A), ptr(b), ptr(m), ptr(r),
                                             ptr(xc), ptr(st))
            elif call == "bbox":
                lb, ub, st = out((B, d), torch.float64), out((B, d), torch.float64), out((B,), torch.int32)
                rc = lib.plp_bbox_batch_dev(ctx.handle, stream, sizes[0], sizes[1], sizes[2], ptr(A), ptr(b), ptr(m), ptr(lb),
                                            ptr(ub), ptr(st))
            else:
                n, _, _, lo, hi, compact, n1 = sizes
                if not compact:
                    o = out((B, B), torch.uint8)
                    rc = lib.plp_adjacent_pairs_dev(ctx.handle, stream, n, sizes[1], sizes[2], ptr(A), ptr(b), ptr(m), 1e-7, ptr(o))
                elif n1:   # (the cross call takes the whole n1 x (n - n1) range: the table's cross cases are such)
                    o = out((max(hi, 1),), torch.uint8)
                    rc = lib.plp_overlap_cross_dev(ctx.handle, stream, n1, n - n1, sizes[1], sizes[2], ptr(A), ptr(b), ptr(m), 1e-7,
                                                   ptr(o))
                else:
                    o = out((max(hi - lo, 1),), torch.uint8)
                    rc = lib.plp_adjacent_pairs_range_dev(ctx.handle, stream, n, sizes[1], sizes[2], ptr(A), ptr(b), ptr(m), 1e-7,
                                                          lo, hi, ptr(o))
            torch.cuda.synchronize()
        finally:
            for key in names:
                del os.environ[key]
        print("case %s rc %d" % (cid, rc), flush=True)
    assert lib.plp_selftest(ctx.handle, 8, sep_d.ctypes.data, sep_u.ctypes.data) == 0


def short(name):
    return name.replace("(anonymous namespace)::", "").split("(")[0].replace("void ", "").replace("plp::", "")


def reduce_trace(directory):
    rows = []
    for f in glob.glob(directory + "/**/*kernel_trace.csv", recursive=True):
        rows += [r for r in csv.DictReader(open(f)) if "plp::" in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    ids = [cid for cid, _ in runnable()]
    cases, k = {}, -1
    for r in rows:
        name = short(r["Kernel_Name"])
        if name == SEPARATOR:
            k += 1
            if k < len(ids):
                cases[ids[k]] = []
            continue
        assert 0 <= k < len(ids), "a kernel outside the separators: %s" % name
        wg = int(r["Workgroup_Size_X"])
        cases[ids[k]].append([name, int(r["Grid_Size_X"]) // wg, wg, int(r["LDS_Block_Size"])])
    assert k == len(ids), "separators: %d, cases: %d" % (k, len(ids))
    return cases


def main():
    if "--worker" in sys.argv[1:]:
        return worker()
    out = [a for a in sys.argv[1:] if not a.startswith("--")][0]
    with tempfile.TemporaryDirectory() as tmp:
        cmd = ["timeout", "-k", "10", str(LIMIT_S), "rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", tmp, "-o", "lp_plan",
               "--", sys.executable, os.path.abspath(__file__), "--worker"] + (["--instances"] if INSTANCES else [])
        log = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        if log.returncode:
            sys.stdout.write(log.stdout[-4000:])
            sys.exit("the traced run ended with status %d" % log.returncode)
        cases = reduce_trace(tmp)
    with open(out, "w") as f:
        json.dump({"cases": cases}, f, indent=0, sort_keys=True)
        f.write("\n")
    print("%d cases, %d launches -> %s" % (len(cases), sum(len(v) for v in cases.values()), out))


if __name__ == "__main__":
    main()
