"""What the host builds of the enumeration kernels (tests/extreme_host.py, tests/hull_host.py, tests/volume_exact_host.py)
share: compiling tests/cabi/*_host.cpp with g++ -ffp-contract=off as a shared object or as a stand-alone program under the
sanitizers, and the small helpers of their callers."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST_FLAGS = ["-std=c++17", "-ffp-contract=off"]


def build(src, so_name, tmpdir):
    """Compiles the host build `src` into tmpdir -> the path of the shared object."""
    out = os.path.join(str(tmpdir), so_name)
    subprocess.check_call(["g++", "-O2"] + HOST_FLAGS + ["-fPIC", "-shared", "-o", out, src])
    return out


def build_program(src, macro, exe_name, tmpdir):
    """The stand-alone program (-D`macro` adds its main()) under -fsanitize=address,undefined -> its path."""
    out = os.path.join(str(tmpdir), exe_name)
    subprocess.check_call(["g++", "-O1", "-g"] + HOST_FLAGS + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                                                              "-fno-omit-frame-pointer", "-D" + macro, "-o", out, src])
    return out


def ptr(a):
    return None if a is None else C.c_void_p(a.ctypes.data)


def keep_word(mask):
    """bool[m] -> the uint64 keep word."""
    return np.uint64(sum(1 << int(i) for i in np.nonzero(mask)[0]))


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.int64), np.ascontiguousarray(b).view(np.int64))


def upper_bound(d, n):
    """The upper-bound theorem, as batch sizes v_max and f_max (written out again: the tests do not ask the code)."""
    return max(1, 2 if d == 1 else n if d == 2 else 2 * n - 4 if d == 3 else n * (n - 3) // 2)
