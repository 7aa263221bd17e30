"""CPU: the ratio-test row loop of the lane kernels (polytope_amd/csrc/plp_lane_lp.hpp: lane::ratio_rows -- one loop for the
walk's pass, its first pass from x' = 0, the first pass of a box LP along an axis, the relaxed redundancy LPs, every share of
the rows) compiled for the HOST and compared with a plain restatement of the formulas it replaced
(tests/cabi/lane_ratio_host.cpp: separate dot products, subtraction, running selects, absolute row numbers) -- bit for bit,
except that the walk's pass forms its slack in one fma chain: there the same row and a.d, the slack within
1e-15 (|beta| + sum |a_j x_j|), another row only where the two best ratios lie within 4 ulp of each other: random 16- and
32-row sets in R^3 and R^4 (and d = 1, 2 embedded), duplicated rows (the lower row wins the tie), sets with no eligible row
(bi = -1, bs / bd untouched), the relaxed form for every row k, the rows cut into 1, 2 and 4 shares and met by the lanes' rule."""
import ctypes as C
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cabi", "lane_ratio_host.cpp")
NAMES = ("sets", "mismatches", "ties", "none", "relaxed", "shares", "axis", "first", "near_ties")


def test_row_loop_equals_the_plain_formulas(tmp_path):
    out = str(tmp_path / "liblane_ratio_host.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-o", out, SRC])
    L = C.CDLL(out)
    L.lane_ratio_check.argtypes = [C.c_longlong, C.c_ulonglong, C.POINTER(C.c_longlong)]
    st = (C.c_longlong * 9)()
    rc = L.lane_ratio_check(100000, 1, st)
    s = dict(zip(NAMES, [int(v) for v in st]))
    print(s)
    assert rc == 0 and s["mismatches"] == 0, s
    # 100 000 sets each in R^3 and R^4 (plus the embedded dimensions), and every family was really there
    assert s["sets"] >= 2 * 100000 and s["ties"] > 1000 and s["none"] > 20000, s
    # (rows whose ratios agree to 4 ulp have no order that survives another sequence of compares or another rounding of the
    # slack: at d = 1 every row with beta = 0 is the same constraint, scaled; nowhere else on random rows)
    assert s["near_ties"] <= s["shares"] // 1000, s
    assert s["relaxed"] > 2 * 100000 * 4 and s["shares"] == 2 * s["sets"] and s["axis"] > 6 * 100000 and s["first"] > 100000, s


def test_row_loop_under_the_address_and_undefined_behaviour_sanitizers(tmp_path):
    """The same checks as a stand-alone program with its own main, built with -fsanitize=address,undefined: every read of
    the strided tile stays inside it, for every share and stride."""
    exe = str(tmp_path / "lane_ratio_san")
    try:
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined",
                               "-fno-sanitize-recover=all", "-DLANE_RATIO_MAIN", "-o", exe, SRC])
    except subprocess.CalledProcessError:
        pytest.fail("g++ could not build with -fsanitize=address,undefined")
    r = subprocess.run([exe, "3000"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "mismatches 0 " in r.stdout, (r.returncode, r.stdout[-400:], r.stderr[-2000:])
