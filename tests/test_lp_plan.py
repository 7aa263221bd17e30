"""CPU: the plans of the stand-alone LP, Chebyshev-ball, bounding-box and pair batches (polytope_amd/csrc/plp_lp_plan.hpp) --
which kernels run a call under which A/B switches, with what grid, workgroup and LDS bytes, and what follows the first launch.
The header is pure host code; it is compiled here with g++ and called through ctypes (tests/cabi/lp_plan_host.cpp).
The table straddles every threshold of the header and covers each switch the GPU tests use.  Its values are the launches the
launchers made when each of them still decided for itself ("try this one, fall through when it declines"), read off that
code, and checked against kernel traces on the device from before and after the plan (profiles/lp_plan_trace_*.json,
scripts/trace_lp_plan.py; the rows with more than a few tens of thousands of members stay CPU-only)."""
import ctypes as C
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("LDS", "LP_WIDE", "LP_1ROW", "CHEBY_WIDE", "CHEBY_1ROW", "CHEBY_RETRY_ALL", "BBOX_LANE", "BBOX_SPLIT", "BBOX_WIDE",
        "BBOX_WSPLIT", "BBOX_WSPLIT_MAXB", "BBOX_WDENSE", "ADJ_WIDE")
CALLS = ("lp", "cheby", "bbox", "pairs")
ENGINES = ("NONE", "EMPTY", "LDS", "WIDE", "GROUP", "GENERAL", "LANE", "SPLIT")
FIELDS = ("engine", "gs", "rows", "nw", "dense", "grid", "block", "lds")

# (call, sizes, {switch: value}) -> (launches in order, figures of the call), (None, None) where the size is refused.
#   sizes:    lp (B, m_max, n); cheby, bbox (B, m_max, d); pairs (n, m_max, d, p_lo, p_hi, compact, cross_n1)
#   launch:   (kernel with its template arguments, workgroups, threads per workgroup, dynamic LDS bytes)
#   figures:  lp (the general kernel's retry pass follows: phase 1 reports `more`,); cheby (force_retry,);
#             bbox (force_retry, hand-over mode); pairs (force_retry, p_lo, p_hi as the kernel gets them)
CASES = [
    (('lp', (1000, 16, 2), {}), ([('lp_r_kernel<2, 4>', 63, 64, 0), ('lp_kernel<2>', 63, 256, 0)], (1,))),
    (('lp', (1000, 16, 3), {}), ([('lp_r_kernel<3, 4>', 63, 64, 0), ('lp_p1_r_kernel<3, 4, 4>', 63, 64, 0), ('lp_kernel<3>', 63, 256, 0)], (1,))),
    (('lp', (1000, 16, 4), {}), ([('lp_r_kernel<4, 4>', 63, 64, 0), ('lp_p1_r_kernel<4, 4, 4>', 63, 64, 0), ('lp_kernel<4>', 63, 256, 0)], (1,))),
    (('lp', (1000, 16, 5), {}), ([('lp_w_kernel<5>', 1000, 64, 0)], (0,))),
    (('lp', (1000, 16, 8), {}), ([('lp_w_kernel<8>', 1000, 64, 0)], (0,))),
    (('lp', (1000, 16, 9), {}), ([('lp_w_kernel<9>', 1000, 64, 0)], (0,))),
    (('lp', (1000, 16, 16), {}), ([('lp_w_kernel<16>', 1000, 64, 0)], (0,))),
    (('lp', (1000, 16, 17), {}), ([('lp_r_kernel<17, 8>', 125, 64, 0), ('lp_kernel<17>', 63, 256, 0)], (1,))),
    (('lp', (1000, 16, 5), {'LP_WIDE': '0'}), ([('lp_r_kernel<5, 4>', 63, 64, 0), ('lp_kernel<5>', 63, 256, 0)], (1,))),
    (('lp', (1000, 16, 8), {'LP_WIDE': '0'}), ([('lp_r_kernel<8, 4>', 63, 64, 0), ('lp_kernel<8>', 63, 256, 0)], (1,))),
    (('lp', (1000, 16, 9), {'LP_WIDE': '0'}), ([('lp_r_kernel<9, 8>', 125, 64, 0), ('lp_kernel<9>', 63, 256, 0)], (1,))),
    (('lp', (1000, 16, 16), {'LP_WIDE': '0'}), ([('lp_r_kernel<16, 8>', 125, 64, 0), ('lp_kernel<16>', 63, 256, 0)], (1,))),
    (('lp', (1000, 16, 4), {'LP_WIDE': '1'}), ([('lp_r_kernel<4, 4>', 63, 64, 0), ('lp_p1_r_kernel<4, 4, 4>', 63, 64, 0), ('lp_kernel<4>', 63, 256, 0)], (1,))),
    (('lp', (1000, 16, 8), {'LP_WIDE': ''}), ([('lp_r_kernel<8, 4>', 63, 64, 0), ('lp_kernel<8>', 63, 256, 0)], (1,))),
    (('lp', (1000, 0, 3), {}), ([('lp_kernel<3>', 32, 256, 0)], (0,))),
    (('lp', (1000, 8, 3), {}), ([('lp_r_kernel<3, 4>', 63, 64, 0), ('lp_p1_r_kernel<3, 4, 4>', 63, 64, 0), ('lp_kernel<3>', 32, 256, 0)], (1,))),
    (('lp', (1000, 9, 3), {}), ([('lp_r_kernel<3, 4>', 63, 64, 0), ('lp_p1_r_kernel<3, 4, 4>', 63, 64, 0), ('lp_kernel<3>', 63, 256, 0)], (1,))),
    (('lp', (1000, 17, 3), {}), ([('lp_r_kernel<3, 8>', 125, 64, 0), ('lp_p1_r_kernel<3, 8, 4>', 125, 64, 0), ('lp_kernel<3>', 125, 256, 0)], (1,))),
    (('lp', (1000, 32, 3), {}), ([('lp_r_kernel<3, 8>', 125, 64, 0), ('lp_p1_r_kernel<3, 8, 4>', 125, 64, 0), ('lp_kernel<3>', 125, 256, 0)], (1,))),
    (('lp', (1000, 33, 3), {}), ([('lp_r_kernel<3, 16>', 250, 64, 0), ('lp_p1_r_kernel<3, 16, 4>', 250, 64, 0), ('lp_kernel<3>', 250, 256, 0)], (1,))),
    (('lp', (1000, 64, 3), {}), ([('lp_r_kernel<3, 16>', 250, 64, 0), ('lp_p1_r_kernel<3, 16, 4>', 250, 64, 0), ('lp_kernel<3>', 250, 256, 0)], (1,))),
    (('lp', (1000, 65, 3), {}), ([('lp_lds_kernel', 1000, 64, 5120)], (0,))),
    (('lp', (1000, 0, 8), {}), ([('lp_kernel<8>', 32, 256, 0)], (0,))),
    (('lp', (1000, 32, 12), {'LP_WIDE': '0'}), ([('lp_r_kernel<12, 16>', 250, 64, 0), ('lp_kernel<12>', 125, 256, 0)], (1,))),
    (('lp', (1000, 33, 12), {'LP_WIDE': '0'}), ([('lp_r_kernel<12, 32>', 500, 64, 0), ('lp_kernel<12>', 250, 256, 0)], (1,))),
    (('lp', (1000, 64, 17), {}), ([('lp_r_kernel<17, 32>', 500, 64, 0), ('lp_kernel<17>', 250, 256, 0)], (1,))),
    (('lp', (1000, 65, 17), {}), ([('lp_lds_kernel', 1000, 64, 12400)], (0,))),
    (('lp', (4, 2545, 4), {}), ([('lp_lds_kernel', 4, 64, 163840)], (0,))),
    (('lp', (4, 2546, 4), {}), (None, None)),
    (('lp', (40000, 70, 4), {}), ([('lp_lds_kernel', 30720, 64, 5440)], (0,))),
    (('lp', (1000, 16, 3), {'LP_1ROW': '1'}), ([('lp_kernel<3>', 63, 256, 0)], (0,))),
    (('lp', (1000, 16, 8), {'LP_1ROW': '1'}), ([('lp_kernel<8>', 63, 256, 0)], (0,))),
    (('lp', (1000, 16, 8), {'LP_1ROW': '1', 'LP_WIDE': '1'}), ([('lp_w_kernel<8>', 1000, 64, 0)], (0,))),
    (('lp', (1000, 16, 3), {'LP_1ROW': '0'}), ([('lp_r_kernel<3, 4>', 63, 64, 0), ('lp_p1_r_kernel<3, 4, 4>', 63, 64, 0), ('lp_kernel<3>', 63, 256, 0)], (1,))),
    (('lp', (1000, 16, 3), {'LDS': '1'}), ([('lp_lds_kernel', 1000, 64, 1984)], (0,))),
    (('lp', (1000, 16, 3), {'LDS': '0'}), ([('lp_r_kernel<3, 4>', 63, 64, 0), ('lp_p1_r_kernel<3, 4, 4>', 63, 64, 0), ('lp_kernel<3>', 63, 256, 0)], (1,))),
    (('lp', (33025, 16, 3), {'LDS': '1'}), ([('lp_lds_kernel', 32768, 64, 1984)], (0,))),
    (('lp', (1000, 0, 3), {'LDS': '1'}), ([('lp_lds_kernel', 1000, 64, 1024)], (0,))),
    (('lp', (32768, 16, 3), {}), ([('lp_r_kernel<3, 4>', 2048, 64, 0), ('lp_p1_r_kernel<3, 4, 4>', 2048, 64, 0), ('lp_kernel<3>', 2048, 256, 0)], (1,))),
    (('lp', (32769, 16, 3), {}), ([('lp_r_kernel<3, 4>', 2049, 64, 0), ('lp_p1_r_kernel<3, 4, 4>', 2049, 64, 0), ('lp_kernel<3>', 2048, 256, 0)], (1,))),
    (('lp', (257, 40, 17), {}), ([('lp_r_kernel<17, 32>', 129, 64, 0), ('lp_kernel<17>', 65, 256, 0)], (1,))),
    (('lp', (1, 24, 8), {}), ([('lp_w_kernel<8>', 1, 64, 0)], (0,))),
    (('lp', (2147483647, 16, 8), {}), ([('lp_w_kernel<8>', 2147483647, 64, 0)], (0,))),
    (('lp', (2147483648, 16, 8), {}), ([('lp_r_kernel<8, 4>', 134217728, 64, 0), ('lp_kernel<8>', 2048, 256, 0)], (1,))),
    (('lp', (8589934588, 64, 3), {}), ([('lp_r_kernel<3, 16>', 2147483647, 64, 0), ('lp_p1_r_kernel<3, 16, 4>', 2147483647, 64, 0), ('lp_kernel<3>', 2048, 256, 0)], (1,))),
    (('lp', (8589934589, 64, 3), {}), ([('lp_kernel<3>', 1048576, 256, 0)], (0,))),
    (('lp', (4294967295, 64, 9), {}), ([('lp_kernel<9>', 1048576, 256, 0)], (0,))),
    (('lp', (2147483648, 16, 3), {'LP_1ROW': '1'}), ([('lp_kernel<3>', 1048576, 256, 0)], (0,))),
    (('lp', (1000, 16, 18), {}), (None, None)),
    (('lp', (1000, 16, 0), {}), (None, None)),
    (('lp', (1000, -1, 3), {}), (None, None)),
    (('cheby', (4096, 32, 5), {}), ([('cheby_w_kernel<5>', 4096, 64, 0)], (0,))),
    (('cheby', (4097, 32, 5), {}), ([('cheby_r_kernel<5, 8>', 513, 64, 0)], (0,))),
    (('cheby', (4097, 33, 5), {}), ([('cheby_w_kernel<5>', 4097, 64, 0)], (0,))),
    (('cheby', (4096, 32, 4), {}), ([('cheby_r_kernel<4, 8>', 512, 64, 0)], (0,))),
    (('cheby', (4097, 33, 4), {}), ([('cheby_r_kernel<4, 16>', 1025, 64, 0)], (0,))),
    (('cheby', (4096, 64, 4), {}), ([('cheby_r_kernel<4, 16>', 1024, 64, 0)], (0,))),
    (('cheby', (257, 16, 3), {}), ([('cheby_r_kernel<3, 4>', 17, 64, 0)], (0,))),
    (('cheby', (257, 24, 9), {}), ([('cheby_w_kernel<9>', 257, 64, 0)], (0,))),
    (('cheby', (257, 24, 9), {'CHEBY_WIDE': '0'}), ([('cheby_r_kernel<9, 16>', 65, 64, 0)], (0,))),
    (('cheby', (257, 40, 9), {'CHEBY_WIDE': '0'}), ([('cheby_r_kernel<9, 32>', 129, 64, 0)], (0,))),
    (('cheby', (20000, 16, 5), {'CHEBY_WIDE': '1'}), ([('cheby_w_kernel<5>', 20000, 64, 0)], (0,))),
    (('cheby', (1000, 16, 4), {'CHEBY_WIDE': '1'}), ([('cheby_r_kernel<4, 4>', 63, 64, 0)], (0,))),
    (('cheby', (1000, 40, 6), {'CHEBY_WIDE': ''}), ([('cheby_r_kernel<6, 16>', 250, 64, 0)], (0,))),
    (('cheby', (5000, 16, 16), {}), ([('cheby_r_kernel<16, 8>', 625, 64, 0)], (0,))),
    (('cheby', (5000, 8, 16), {}), ([('cheby_r_kernel<16, 4>', 313, 64, 0)], (0,))),
    (('cheby', (5000, 9, 8), {}), ([('cheby_r_kernel<8, 4>', 313, 64, 0)], (0,))),
    (('cheby', (257, 16, 3), {'CHEBY_1ROW': '1'}), ([('cheby_kernel<3>', 17, 256, 0)], (0,))),
    (('cheby', (257, 40, 9), {'CHEBY_1ROW': '1'}), ([('cheby_w_kernel<9>', 257, 64, 0)], (0,))),
    (('cheby', (257, 40, 9), {'CHEBY_1ROW': '1', 'CHEBY_WIDE': '0'}), ([('cheby_kernel<9>', 65, 256, 0)], (0,))),
    (('cheby', (5000, 16, 3), {'CHEBY_RETRY_ALL': '1'}), ([('cheby_r_kernel<3, 4>', 313, 64, 0)], (1,))),
    (('cheby', (1000, 0, 3), {}), ([('cheby_kernel<3>', 32, 256, 0)], (0,))),
    (('cheby', (1000, 0, 6), {}), ([('cheby_kernel<6>', 32, 256, 0)], (0,))),
    (('cheby', (257, 70, 4), {}), ([('cheby_lds_kernel', 257, 64, 5440)], (0,))),
    (('cheby', (257, 16, 3), {'LDS': '1'}), ([('cheby_lds_kernel', 257, 64, 1984)], (0,))),
    (('cheby', (33025, 16, 3), {'LDS': '1'}), ([('cheby_lds_kernel', 32768, 64, 1984)], (0,))),
    (('cheby', (4, 2546, 3), {}), (None, None)),
    (('cheby', (2147483647, 40, 6), {}), ([('cheby_w_kernel<6>', 2147483647, 64, 0)], (0,))),
    (('cheby', (2147483648, 40, 6), {}), ([('cheby_r_kernel<6, 16>', 536870912, 64, 0)], (0,))),
    (('cheby', (34359738353, 16, 3), {}), ([('cheby_kernel<3>', 1048576, 256, 0)], (0,))),
    (('cheby', (1000, 16, 17), {}), (None, None)),
    (('bbox', (257, 16, 3), {}), ([('bbox_lane_kernel<3, 16, 16>', 65, 64, 2560)], (0, 2))),
    (('bbox', (14000, 16, 3), {}), ([('bbox_lane_kernel<3, 16, 16>', 3500, 64, 2560)], (0, 2))),
    (('bbox', (14001, 16, 3), {}), ([('bbox_lane_kernel<3, 8, 16>', 1751, 64, 5120)], (0, 2))),
    (('bbox', (40000, 16, 2), {}), ([('bbox_lane_kernel<2, 8, 16>', 5000, 64, 4096)], (0, 2))),
    (('bbox', (40001, 16, 2), {}), ([('bbox_lane_kernel<2, 4, 16>', 2501, 64, 8192)], (0, 2))),
    (('bbox', (16000, 24, 3), {}), ([('bbox_lane_kernel<3, 16, 32>', 4000, 64, 5120)], (0, 2))),
    (('bbox', (16001, 24, 3), {}), ([('bbox_lane_kernel<3, 8, 32>', 2001, 64, 10240)], (0, 2))),
    (('bbox', (257, 32, 3), {}), ([('bbox_lane_kernel<3, 16, 32>', 65, 64, 5120)], (0, 2))),
    (('bbox', (257, 33, 3), {}), ([('bbox_split_kernel<3, 16>', 257, 64, 0)], (0, 1))),
    (('bbox', (257, 16, 4), {}), ([('bbox_split_kernel<4, 4>', 257, 64, 0)], (0, 1))),
    (('bbox', (257, 16, 3), {'BBOX_LANE': '0'}), ([('bbox_split_kernel<3, 4>', 257, 64, 0)], (0, 1))),
    (('bbox', (257, 16, 3), {'BBOX_LANE': '0', 'BBOX_SPLIT': '0'}), ([('bbox_r_kernel<3, 4>', 17, 64, 0)], (0, 1))),
    (('bbox', (257, 16, 3), {'BBOX_SPLIT': ''}), ([('bbox_split_kernel<3, 4>', 257, 64, 0)], (0, 1))),
    (('bbox', (257, 16, 3), {'BBOX_LANE': '1', 'BBOX_SPLIT': '1'}), ([('bbox_split_kernel<3, 4>', 257, 64, 0)], (0, 1))),
    (('bbox', (4096, 16, 4), {}), ([('bbox_split_kernel<4, 4>', 4096, 64, 0)], (0, 1))),
    (('bbox', (4097, 16, 4), {}), ([('bbox_r_kernel<4, 4>', 257, 64, 0)], (0, 1))),
    (('bbox', (4096, 32, 4), {}), ([('bbox_split_kernel<4, 8>', 4096, 64, 0)], (0, 1))),
    (('bbox', (4097, 32, 4), {}), ([('bbox_r_kernel<4, 8>', 513, 64, 0)], (0, 1))),
    (('bbox', (1024, 40, 4), {}), ([('bbox_split_kernel<4, 16>', 1024, 64, 0)], (0, 1))),
    (('bbox', (1025, 40, 4), {}), ([('bbox_r_kernel<4, 16>', 257, 64, 0)], (0, 1))),
    (('bbox', (20000, 16, 4), {'BBOX_SPLIT': '1'}), ([('bbox_split_kernel<4, 4>', 20000, 64, 0)], (0, 1))),
    (('bbox', (257, 16, 4), {'BBOX_SPLIT': '0'}), ([('bbox_r_kernel<4, 4>', 17, 64, 0)], (0, 1))),
    (('bbox', (2000, 24, 6), {}), ([('bbox_wsplit_kernel<6, 4, true>', 2000, 256, 0)], (0, 1))),
    (('bbox', (2001, 24, 6), {}), ([('bbox_split_kernel<6, 8>', 2001, 64, 0)], (0, 1))),
    (('bbox', (4097, 24, 6), {}), ([('bbox_r_kernel<6, 8>', 513, 64, 0)], (0, 1))),
    (('bbox', (1024, 40, 6), {}), ([('bbox_wsplit_kernel<6, 4, true>', 1024, 256, 0)], (0, 1))),
    (('bbox', (1025, 40, 6), {}), ([('bbox_wsplit_kernel<6, 4, true>', 1025, 256, 0)], (0, 1))),
    (('bbox', (2001, 40, 6), {}), ([('bbox_lazy_kernel<6, true>', 2001, 64, 0)], (0, 1))),
    (('bbox', (2001, 32, 6), {}), ([('bbox_split_kernel<6, 8>', 2001, 64, 0)], (0, 1))),
    (('bbox', (2001, 33, 6), {}), ([('bbox_lazy_kernel<6, true>', 2001, 64, 0)], (0, 1))),
    (('bbox', (1024, 40, 6), {'BBOX_WSPLIT': ''}), ([('bbox_split_kernel<6, 16>', 1024, 64, 0)], (0, 1))),
    (('bbox', (1025, 40, 6), {'BBOX_WSPLIT': ''}), ([('bbox_wsplit_kernel<6, 4, true>', 1025, 256, 0)], (0, 1))),
    (('bbox', (257, 24, 6), {'BBOX_SPLIT': ''}), ([('bbox_split_kernel<6, 8>', 257, 64, 0)], (0, 1))),
    (('bbox', (257, 24, 6), {'BBOX_WIDE': ''}), ([('bbox_split_kernel<6, 8>', 257, 64, 0)], (0, 1))),
    (('bbox', (257, 24, 6), {'BBOX_WIDE': '1', 'BBOX_WDENSE': '1'}), ([('bbox_wsplit_kernel<6, 4, true>', 257, 256, 0)], (0, 1))),
    (('bbox', (257, 24, 6), {'BBOX_WIDE': '1', 'BBOX_WDENSE': '0'}), ([('bbox_wsplit_kernel<6, 4, false>', 257, 256, 0)], (0, 1))),
    (('bbox', (257, 24, 6), {'BBOX_WIDE': '0', 'BBOX_SPLIT': '0'}), ([('bbox_r_kernel<6, 8>', 33, 64, 0)], (0, 1))),
    (('bbox', (5000, 24, 6), {'BBOX_WIDE': '1'}), ([('bbox_lazy_kernel<6, true>', 5000, 64, 0)], (0, 1))),
    (('bbox', (257, 24, 6), {'BBOX_WSPLIT_MAXB': '100'}), ([('bbox_lazy_kernel<6, true>', 257, 64, 0)], (0, 1))),
    (('bbox', (5000, 40, 6), {'BBOX_WSPLIT_MAXB': '5000'}), ([('bbox_wsplit_kernel<6, 4, true>', 5000, 256, 0)], (0, 1))),
    (('bbox', (257, 40, 6), {'BBOX_WSPLIT': '0'}), ([('bbox_split_kernel<6, 16>', 257, 64, 0)], (0, 1))),
    (('bbox', (5000, 40, 6), {'BBOX_WSPLIT': '1'}), ([('bbox_wsplit_kernel<6, 4, true>', 5000, 256, 0)], (0, 1))),
    (('bbox', (257, 24, 6), {'BBOX_WDENSE': ''}), ([('bbox_wsplit_kernel<6, 4, false>', 257, 256, 0)], (0, 1))),
    (('bbox', (257, 24, 5), {'BBOX_WIDE': '1'}), ([('bbox_wsplit_kernel<5, 4, true>', 257, 256, 0)], (0, 1))),
    (('bbox', (257, 24, 4), {'BBOX_WIDE': '1'}), ([('bbox_split_kernel<4, 8>', 257, 64, 0)], (0, 1))),
    (('bbox', (5000, 24, 8), {}), ([('bbox_r_kernel<8, 8>', 625, 64, 0)], (0, 1))),
    (('bbox', (5000, 24, 9), {}), ([('bbox_lazy_kernel<9, true>', 5000, 64, 0)], (0, 1))),
    (('bbox', (5000, 24, 13), {}), ([('bbox_lazy_kernel<13, true>', 5000, 64, 0)], (0, 1))),
    (('bbox', (5000, 24, 14), {}), ([('bbox_lazy_kernel<14, false>', 5000, 64, 0)], (0, 1))),
    (('bbox', (257, 40, 14), {}), ([('bbox_wsplit_kernel<14, 4, false>', 257, 256, 0)], (0, 1))),
    (('bbox', (257, 40, 14), {'BBOX_WDENSE': '1'}), ([('bbox_wsplit_kernel<14, 4, true>', 257, 256, 0)], (0, 1))),
    (('bbox', (257, 24, 9), {'BBOX_WIDE': '0'}), ([('bbox_wsplit_kernel<9, 4, true>', 257, 256, 0)], (0, 1))),
    (('bbox', (5000, 24, 16), {'BBOX_WSPLIT': '1'}), ([('bbox_wsplit_kernel<16, 4, false>', 5000, 256, 0)], (0, 1))),
    (('bbox', (5000, 16, 6), {'CHEBY_RETRY_ALL': '1'}), ([('bbox_r_kernel<6, 4>', 313, 64, 0)], (1, 1))),
    (('bbox', (257, 0, 3), {}), (None, None)),
    (('bbox', (257, 65, 3), {}), (None, None)),
    (('bbox', (257, 16, 17), {}), (None, None)),
    (('bbox', (2147483648, 16, 3), {}), ([('bbox_r_kernel<3, 4>', 134217728, 64, 0)], (0, 1))),
    (('bbox', (2147483648, 40, 6), {}), ([('bbox_r_kernel<6, 16>', 536870912, 64, 0)], (0, 1))),
    (('bbox', (2147483648, 40, 9), {}), (None, None)),
    (('bbox', (34359738353, 16, 4), {}), (None, None)),
    (('pairs', (20, 6, 2, 0, 0, 0, 0), {}), ([('adjacent_r_kernel<2, 4>', 12, 64, 0)], (0, 0, 190))),
    (('pairs', (257, 10, 4, 0, 0, 0, 0), {}), ([('adjacent_r_kernel<4, 8>', 4112, 64, 0)], (0, 0, 32896))),
    (('pairs', (1, 6, 2, 0, 0, 0, 0), {}), ([('adjacent_r_kernel<2, 4>', 1, 64, 0)], (0, 0, 0))),
    (('pairs', (1, 6, 12, 0, 0, 0, 0), {}), ([('adjacent_w_kernel<12>', 1, 64, 0)], (0, 0, 0))),
    (('pairs', (100, 16, 5, 0, 0, 0, 0), {}), ([('adjacent_r_kernel<5, 8>', 619, 64, 0)], (0, 0, 4950))),
    (('pairs', (100, 17, 5, 0, 0, 0, 0), {}), ([('adjacent_w_kernel<5>', 4950, 64, 0)], (0, 0, 4950))),
    (('pairs', (100, 32, 4, 0, 0, 0, 0), {}), ([('adjacent_r_kernel<4, 16>', 1238, 64, 0)], (0, 0, 4950))),
    (('pairs', (257, 10, 6, 0, 4096, 1, 0), {}), ([('adjacent_w_kernel<6>', 4096, 64, 0)], (0, 0, 4096))),
    (('pairs', (257, 10, 6, 0, 4097, 1, 0), {}), ([('adjacent_r_kernel<6, 8>', 513, 64, 0)], (0, 0, 4097))),
    (('pairs', (257, 10, 6, 3, 32894, 1, 0), {}), ([('adjacent_r_kernel<6, 8>', 4112, 64, 0)], (0, 3, 32894))),
    (('pairs', (20, 14, 5, 0, 0, 0, 0), {}), ([('adjacent_w_kernel<5>', 190, 64, 0)], (0, 0, 190))),
    (('pairs', (257, 14, 5, 3, 32894, 1, 0), {}), ([('adjacent_r_kernel<5, 8>', 4112, 64, 0)], (0, 3, 32894))),
    (('pairs', (257, 20, 8, 0, 0, 0, 0), {'ADJ_WIDE': '0'}), ([('adjacent_r_kernel<8, 16>', 8224, 64, 0)], (0, 0, 32896))),
    (('pairs', (100, 20, 9, 0, 0, 0, 0), {'ADJ_WIDE': '0'}), ([('adjacent_w_kernel<9>', 4950, 64, 0)], (0, 0, 4950))),
    (('pairs', (257, 28, 12, 0, 0, 0, 0), {}), ([('adjacent_w_kernel<12>', 32896, 64, 0)], (0, 0, 32896))),
    (('pairs', (257, 10, 4, 0, 0, 0, 0), {'ADJ_WIDE': '1'}), ([('adjacent_r_kernel<4, 8>', 4112, 64, 0)], (0, 0, 32896))),
    (('pairs', (257, 10, 5, 0, 0, 0, 0), {'ADJ_WIDE': '1'}), ([('adjacent_w_kernel<5>', 32896, 64, 0)], (0, 0, 32896))),
    (('pairs', (257, 10, 5, 0, 0, 0, 0), {'ADJ_WIDE': ''}), ([('adjacent_r_kernel<5, 8>', 4112, 64, 0)], (0, 0, 32896))),
    (('pairs', (257, 10, 3, 0, 0, 0, 0), {'CHEBY_RETRY_ALL': '1'}), ([('adjacent_r_kernel<3, 8>', 4112, 64, 0)], (1, 0, 32896))),
    (('pairs', (0, 6, 2, 0, 0, 0, 0), {}), ([], (0, 0, 0))),
    (('pairs', (20, 6, 2, 7, 7, 1, 0), {}), ([], (0, 7, 7))),
    (('pairs', (20, 6, 2, 7, 8, 1, 0), {}), ([('adjacent_r_kernel<2, 4>', 1, 64, 0)], (0, 7, 8))),
    (('pairs', (10, 6, 2, 0, 21, 1, 3), {}), ([('adjacent_r_kernel<2, 4>', 2, 64, 0)], (0, 0, 21))),
    (('pairs', (257, 10, 6, 0, 14706, 1, 86), {}), ([('adjacent_r_kernel<6, 8>', 1839, 64, 0)], (0, 0, 14706))),
    (('pairs', (10, 6, 2, 0, 21, 0, 3), {}), (None, None)),
    (('pairs', (20, 6, 2, 0, 191, 1, 0), {}), (None, None)),
    (('pairs', (20, 6, 2, 8, 7, 1, 0), {}), (None, None)),
    (('pairs', (20, 33, 2, 0, 0, 0, 0), {}), (None, None)),
    (('pairs', (20, 6, 17, 0, 0, 0, 0), {}), (None, None)),
    (('pairs', (20, 0, 2, 0, 0, 0, 0), {}), (None, None)),
]


def kernel_name(call, dim, L, pos):
    """The kernel a planned launch stands for, as a trace names it."""
    e, t = L["engine"], "true" if L["dense"] else "false"
    if call == "lp":
        return {"LDS": "lp_lds_kernel", "WIDE": "lp_w_kernel<%d>" % dim, "GENERAL": "lp_kernel<%d>" % dim,
                "GROUP": ("lp_p1_r_kernel<%d, %d, %d>" % (dim, L["gs"], L["rows"])) if pos else "lp_r_kernel<%d, %d>" % (dim, L["gs"])}[e]
    if call == "cheby":
        return {"LDS": "cheby_lds_kernel", "WIDE": "cheby_w_kernel<%d>" % dim, "GENERAL": "cheby_kernel<%d>" % dim,
                "GROUP": "cheby_r_kernel<%d, %d>" % (dim, L["gs"])}[e]
    if call == "bbox":
        return {"LANE": "bbox_lane_kernel<%d, %d, %d>" % (dim, L["gs"], L["rows"]),
                "WIDE": ("bbox_wsplit_kernel<%d, 4, %s>" if L["nw"] == 4 else "bbox_lazy_kernel<%d, %s>") % (dim, t),
                "SPLIT": "bbox_split_kernel<%d, %d>" % (dim, L["gs"]), "GROUP": "bbox_r_kernel<%d, %d>" % (dim, L["gs"])}[e]
    return {"WIDE": "adjacent_w_kernel<%d>" % dim, "GROUP": "adjacent_r_kernel<%d, %d>" % (dim, L["gs"])}[e]


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("plan") / "liblp_plan.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-fPIC", "-shared", "-o", out,
                           os.path.join(ROOT, "tests", "cabi", "lp_plan_host.cpp")])
    lib = C.CDLL(out)
    lib.lp_plan.argtypes = [C.c_int, C.POINTER(C.c_longlong), C.POINTER(C.c_char_p), C.POINTER(C.c_longlong)]
    lib.lp_plan.restype = None

    def run(call, sizes, env):
        """-> (list of launches as dicts by FIELDS, or None when refused; the three figures of the call)"""
        assert set(env) <= set(KEYS)
        arr = (C.c_char_p * len(KEYS))(*[(env[k].encode() if k in env else None) for k in KEYS])
        a = (C.c_longlong * 7)(*sizes)
        o = (C.c_longlong * (4 + 3 * len(FIELDS)))()
        lib.lp_plan(CALLS.index(call), a, arr, o)
        if o[0] < 0:
            return None, None
        launches = [dict(zip(FIELDS, o[4 + k * len(FIELDS):4 + (k + 1) * len(FIELDS)])) for k in range(o[0])]
        for L in launches:
            L["engine"] = ENGINES[L["engine"]]
        return launches, tuple(o[1:4])
    run.lib = lib   # (lp_plan_thresholds, lp_plan_sweep: tests/instance_cases.py)
    return run


def planned(plan, call, sizes, env):
    """A plan in the vocabulary of the table."""
    launches, figures = plan(call, sizes, env)
    if launches is None:
        return None, None
    rows = [(kernel_name(call, sizes[2], L, k), L["grid"], L["block"], L["lds"]) for k, L in enumerate(launches)]
    return rows, figures[:{"lp": 1, "cheby": 1, "bbox": 2, "pairs": 3}[call]]


def case_id(case):
    call, sizes, env = case
    return "%s-%s-%s" % (call, "-".join(str(s) for s in sizes), ",".join("%s=%s" % kv for kv in sorted(env.items())) or "default")


@pytest.mark.parametrize("case,want", CASES, ids=[case_id(c[0]) for c in CASES])
def test_plan_table(plan, case, want):
    assert planned(plan, *case) == want


def test_tile_shapes(plan):
    """What a kernel's name does not show: the general kernels get 8 / 16 / 32 / 64 lanes per LP by the row count, the lane
    groups four rows per lane up to d = 8 and two beyond, in groups that hold the rows."""
    for (call, sizes, env), (want, _) in CASES:
        launches, _ = plan(call, sizes, env)
        for L in launches or ():
            rows = 2 * sizes[1] if call == "pairs" else sizes[1]
            if L["engine"] == "GENERAL":
                assert L["gs"] == (8 if rows <= 8 else 16 if rows <= 16 else 32 if rows <= 32 else 64), (call, sizes, L)
            if L["engine"] in ("GROUP", "SPLIT"):
                assert L["rows"] == (4 if sizes[2] <= 8 else 2) and L["gs"] * L["rows"] >= rows, (call, sizes, L)
                assert L["gs"] == 4 or (L["gs"] // 2) * L["rows"] < rows, (call, sizes, L)


def test_switch_presence(plan):
    """PLP_BBOX_SPLIT, PLP_BBOX_WIDE and PLP_BBOX_WSPLIT count as set whatever their value, an empty one included."""
    lane = planned(plan, "bbox", (257, 16, 3), {})[0][0][0]
    assert lane.startswith("bbox_lane_kernel")
    for v in ("", "x", "0"):
        assert not planned(plan, "bbox", (257, 16, 3), {"BBOX_SPLIT": v})[0][0][0].startswith("bbox_lane_kernel"), v
    for k in ("BBOX_SPLIT", "BBOX_WIDE", "BBOX_WSPLIT"):
        assert planned(plan, "bbox", (257, 24, 6), {})[0][0][0].startswith("bbox_wsplit_kernel")
        assert planned(plan, "bbox", (257, 24, 6), {k: ""})[0][0][0].startswith("bbox_split_kernel"), k


TRACES = [os.path.join(ROOT, "profiles", "lp_plan_trace_%s.json" % w) for w in ("before", "after")]


def test_traces_agree_with_the_table():
    """The kernel traces of scripts/trace_lp_plan.py, taken on the device with the launchers that decided for themselves and
    with the plan: identical, and for every case they hold the launches of the table -- kernel, workgroups, threads per
    workgroup.  (The LDS bytes of a trace are a kernel's static arrays only: compared between the traces, not with the table.)
    The retry pass of the generic LPs is in the traces as in the table: the device-pointer call launches both phases."""
    before, after = (json.load(open(f))["cases"] for f in TRACES)
    assert before == after
    table = {case_id(c): w for c, w in CASES}
    assert set(before) <= set(table) and len(before) >= 120
    for cid, got in before.items():
        want = table[cid][0] or []
        assert [tuple(g[:3]) for g in got] == [w[:3] for w in want], cid
