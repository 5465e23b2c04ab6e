"""The polyphase resize (lgpu_resize, the default lgpu_chain) on every kernel its planner can choose.

resize.hip picks one of five kernel families per call -- k_half8s, k_sep2<nph>, k_sep2p<nph, 0, 4>, k_sep2p<1, kb, 4> on the matrix cores, k_separable<0, 0>, or the
two generic passes -- from the tap counts, sw & 3, sw % dw, pointer and pitch alignment and LDS budgets.  lgpu_debug_resize_plan answers, on the host and through the
very functions the launches use, which one a call takes.  ROWS is a table of small geometries with the plan each is expected to take:

  CPU  every row's plan is the one written here; the (path, parameter) pairs of the table are exactly the set the planner can return (REACHABLE, written out below),
       so deleting a row or adding a path to the planner fails; the rows keep to the shape rules (two tile columns with a partial last one, two tile rows with a
       partial last one, windows clamped at all four frame borders)
  GPU  every row: the plan with the real pointers, then lgpu_resize == orc_resize byte for byte, guard row and row padding untouched; one row per (path, nph / kb)
       through lgpu_chain with three tracks, the byte swap, a blend, a LUT; 200 random geometries as the gdk-pixbuf backend has

The spec is integer-exact: no tolerance anywhere.
"""
import ctypes
from collections import namedtuple

import numpy as np
import pytest

from lives_amd import lib
from oracle import pyoracle as po
from tests.util import align, dev, host

P = po.P
gpu_mark = pytest.mark.gpu

Row = namedtuple("Row", "name sw sh dw dh psize interp force ipad path plan")
PLAN_FIELDS = ("kernel", "nth", "ntv", "nph", "npv", "th", "th_start", "sht", "swt", "lds", "mh_r", "mh_c0", "mh_kb", "tiles_x", "tiles_y", "vec", "xoff")

# name, sw, sh, dw, dh, psize, interp, SEP2P_FORCE, extra source pitch bytes, path, PLAN_FIELDS.  Source rows: sw * psize rounded up to 16 bytes + the extra
# bytes; destination rows: dw * psize rounded up to 16 + 16 bytes of padding; frames 16-byte aligned (pitches()).  The plans were taken from the query.
ROWS = [Row(*r) for r in [
    ("half8s_bicubic", 130, 36, 65, 18, 4, 3, 0, 0, "HALF8S", (1, 8, 8, 4, 5, 16, 16, 0, 0, 71904, 0, 0, 0, 2, 2, 0, 1)),
    ("half8s_bilinear", 134, 44, 67, 22, 4, 2, 0, 0, "HALF8S", (0, 4, 4, 2, 3, 16, 16, 0, 0, 71904, 0, 0, 0, 2, 2, 0, 1)),
    ("half8s_bicubic_xoff0", 130, 36, 65, 18, 4, 3, 0, 8, "HALF8S", (1, 8, 8, 4, 5, 16, 16, 0, 0, 71904, 0, 0, 0, 2, 2, 0, 0)),
    ("sep2_1", 40, 36, 65, 18, 4, 2, 0, 0, "SEP2", (0, 2, 4, 1, 3, 16, 16, 38, 44, 26656, 0, 0, 0, 2, 2, 1, 0)),
    ("sep2_2", 100, 50, 67, 37, 4, 2, 0, 0, "SEP2", (0, 3, 3, 2, 2, 16, 16, 28, 104, 26432, 0, 0, 0, 2, 3, 1, 0)),
    ("sep2_3", 90, 50, 67, 37, 4, 3, 0, 0, "SEP2", (1, 6, 6, 3, 4, 16, 16, 28, 96, 25664, 0, 0, 0, 2, 3, 1, 0)),
    ("sep2_3_lanczos_up", 41, 30, 67, 75, 4, 3, 0, 0, "SEP2", (2, 6, 6, 3, 4, 32, 32, 22, 48, 16384, 0, 0, 0, 2, 3, 1, 0)),
    ("sep2_4", 98, 36, 65, 18, 4, 3, 0, 0, "SEP2", (1, 7, 8, 4, 5, 16, 16, 42, 108, 40288, 0, 0, 0, 2, 2, 1, 0)),
    ("sep2_5_halved", 147, 130, 65, 37, 4, 3, 0, 0, "SEP2", (1, 10, 15, 5, 8, 8, 16, 44, 156, 50528, 0, 0, 0, 2, 5, 1, 0)),
    ("sep2_5_unvec", 131, 36, 65, 18, 4, 3, 0, 4, "SEP2", (1, 9, 8, 5, 5, 16, 16, 42, 140, 45664, 0, 0, 0, 2, 2, 0, 0)),
    ("sep2_6", 163, 36, 65, 18, 4, 3, 0, 0, "SEP2", (1, 11, 8, 6, 5, 16, 16, 42, 172, 51040, 0, 0, 0, 2, 2, 1, 0)),
    ("sep2_7", 196, 36, 65, 18, 4, 3, 0, 0, "SEP2", (1, 13, 8, 7, 5, 16, 16, 42, 208, 57088, 0, 0, 0, 2, 2, 1, 0)),
    ("sep2_7_th2", 196, 300, 65, 37, 4, 3, 0, 0, "SEP2", (1, 13, 33, 7, 17, 2, 16, 44, 208, 59536, 0, 0, 0, 2, 19, 1, 0)),
    ("sep2_8", 228, 36, 65, 18, 4, 3, 0, 0, "SEP2", (1, 15, 8, 8, 5, 16, 16, 42, 240, 62464, 0, 0, 0, 2, 2, 1, 0)),
    ("sep2_10", 330, 100, 66, 37, 4, 3, 0, 0, "SEP2", (1, 20, 11, 10, 6, 8, 16, 34, 336, 63584, 0, 0, 0, 2, 5, 1, 0)),
    ("sep2_10_lanczos", 196, 30, 65, 75, 4, 3, 0, 0, "SEP2", (2, 19, 6, 10, 4, 32, 32, 22, 212, 30816, 0, 0, 0, 2, 3, 1, 0)),
    ("sep2_12", 402, 100, 67, 37, 4, 3, 0, 0, "SEP2", (1, 24, 11, 12, 6, 8, 16, 34, 408, 73376, 0, 0, 0, 2, 5, 1, 0)),
    ("sep2_12_lanczos", 239, 30, 65, 75, 4, 3, 0, 0, "SEP2", (2, 23, 6, 12, 4, 32, 32, 22, 260, 35040, 0, 0, 0, 2, 3, 1, 0)),
    ("sep2p_1", 40, 36, 65, 18, 4, 2, 1, 0, "SEP2P", (0, 2, 4, 1, 3, 16, 16, 38, 44, 35232, 0, 0, 0, 2, 2, 1, 0)),
    ("sep2p_2", 68, 36, 65, 18, 4, 2, 1, 0, "SEP2P", (0, 3, 4, 2, 3, 16, 16, 38, 76, 45472, 0, 0, 0, 2, 2, 1, 0)),
    ("sep2p_3", 88, 50, 67, 37, 4, 3, 1, 0, "SEP2P", (1, 6, 6, 3, 4, 16, 16, 28, 92, 38336, 0, 0, 0, 2, 3, 1, 0)),
    ("sep2p_4", 100, 36, 65, 18, 4, 3, 1, 0, "SEP2P", (1, 7, 8, 4, 5, 16, 16, 42, 108, 62048, 0, 0, 0, 2, 2, 1, 0)),
    ("sep2p_5", 132, 36, 65, 18, 4, 3, 1, 0, "SEP2P", (1, 9, 8, 5, 5, 16, 16, 42, 140, 73312, 0, 0, 0, 2, 2, 1, 0)),
    ("sep2p_5_halved", 160, 36, 65, 18, 4, 3, 1, 0, "SEP2P", (1, 10, 8, 5, 5, 8, 16, 26, 168, 52384, 0, 0, 0, 2, 3, 1, 0)),
    ("sep2p_6", 164, 36, 65, 18, 4, 3, 1, 0, "SEP2P", (1, 11, 8, 6, 5, 8, 16, 26, 172, 53728, 0, 0, 0, 2, 3, 1, 0)),
    ("sep2p_6_lanczos", 112, 30, 65, 75, 4, 3, 1, 0, "SEP2P", (2, 11, 6, 6, 4, 32, 32, 22, 120, 37856, 0, 0, 0, 2, 3, 1, 0)),
    ("sep2p_7", 196, 36, 65, 18, 4, 3, 1, 0, "SEP2P", (1, 13, 8, 7, 5, 8, 16, 26, 208, 61728, 0, 0, 0, 2, 3, 1, 0)),
    ("sep2p_8", 228, 36, 65, 18, 4, 3, 1, 0, "SEP2P", (1, 15, 8, 8, 5, 8, 16, 26, 240, 68896, 0, 0, 0, 2, 3, 1, 0)),
    ("sep2p_10", 332, 100, 67, 37, 4, 3, 1, 0, "SEP2P", (1, 20, 11, 10, 6, 4, 16, 22, 336, 76864, 0, 0, 0, 2, 10, 1, 0)),
    ("sep2p_10_th2", 320, 110, 65, 37, 4, 3, 1, 0, "SEP2P", (1, 20, 12, 10, 7, 2, 16, 18, 332, 63328, 0, 0, 0, 2, 19, 1, 0)),
    ("sep2p_12", 400, 100, 67, 37, 4, 3, 1, 0, "SEP2P", (1, 24, 11, 12, 6, 2, 16, 18, 404, 74704, 0, 0, 0, 2, 19, 1, 0)),
    ("sep2p_12_lanczos", 240, 30, 65, 75, 4, 3, 1, 0, "SEP2P", (2, 23, 6, 12, 4, 32, 32, 22, 260, 65568, 0, 0, 0, 2, 3, 1, 0)),
    ("mfma_kb1_bilinear", 132, 100, 66, 37, 4, 2, 0, 0, "SEP2P_MFMA", (0, 4, 6, 2, 4, 8, 16, 28, 136, 46848, 2, 3, 1, 2, 5, 1, 0)),
    ("mfma_kb1_bicubic", 260, 150, 130, 50, 4, 3, 0, 0, "SEP2P_MFMA", (1, 8, 12, 4, 7, 8, 16, 36, 136, 59968, 2, 1, 1, 3, 7, 1, 0)),
    ("mfma_kb2_bilinear_r3", 204, 50, 68, 37, 4, 2, 0, 0, "SEP2P_MFMA", (0, 6, 3, 3, 2, 16, 16, 28, 200, 61248, 3, 3, 2, 2, 3, 1, 0)),
    ("mfma_kb2_bilinear_r4", 260, 50, 65, 37, 4, 2, 0, 0, "SEP2P_MFMA", (0, 8, 3, 4, 2, 16, 16, 28, 264, 75584, 4, 2, 2, 2, 3, 1, 0)),
    ("mfma_kb2_bilinear_r5", 340, 50, 68, 37, 4, 2, 0, 0, "SEP2P_MFMA", (0, 10, 3, 5, 2, 8, 16, 16, 328, 51904, 5, 2, 2, 2, 5, 1, 0)),
    ("mfma_kb2_bilinear_r6", 396, 36, 66, 18, 4, 2, 0, 0, "SEP2P_MFMA", (0, 12, 4, 6, 3, 4, 16, 14, 392, 52704, 6, 1, 2, 2, 5, 1, 0)),
    ("mfma_kb2_bilinear_r6_up", 396, 30, 66, 75, 4, 2, 0, 0, "SEP2P_MFMA", (0, 12, 2, 6, 2, 32, 32, 18, 392, 68000, 6, 1, 2, 2, 3, 1, 0)),
    ("mfma_kb2_bicubic_r3", 204, 50, 68, 37, 4, 3, 0, 0, "SEP2P_MFMA", (1, 12, 6, 6, 4, 16, 16, 28, 204, 62400, 3, 0, 2, 2, 3, 1, 0)),
    ("mfma_kb2_bicubic_r4", 260, 36, 65, 18, 4, 3, 0, 0, "SEP2P_MFMA", (1, 16, 8, 8, 5, 8, 16, 26, 272, 71968, 4, 2, 2, 2, 3, 1, 0)),
    ("sep2_8_mfma_declined", 260, 130, 65, 37, 4, 3, 0, 0, "SEP2", (1, 16, 15, 8, 8, 8, 16, 44, 272, 70944, 0, 0, 0, 2, 5, 1, 0)),
    ("mfma_kb2_bicubic_r4_forced_th2", 260, 130, 65, 37, 4, 3, 1, 0, "SEP2P_MFMA", (1, 16, 15, 8, 8, 2, 16, 22, 272, 60912, 4, 2, 2, 2, 19, 1, 0)),
    ("mfma_kb2_lanczos_r2", 260, 60, 130, 90, 4, 3, 0, 0, "SEP2P_MFMA", (2, 12, 6, 6, 4, 32, 32, 30, 144, 52960, 2, 3, 2, 3, 3, 1, 0)),
    ("separable_nph9", 289, 36, 65, 18, 4, 3, 0, 0, "SEPARABLE", (1, 18, 8, 9, 5, 8, 16, 22, 304, 38272, 0, 0, 0, 2, 3, 1, 0)),
    ("separable_nph9_unvec", 174, 30, 65, 75, 4, 3, 0, 8, "SEPARABLE", (2, 17, 6, 9, 4, 16, 16, 12, 192, 15616, 0, 0, 0, 2, 5, 0, 0)),
    ("separable_nph11", 326, 36, 65, 18, 4, 3, 0, 0, "SEPARABLE", (1, 21, 8, 11, 5, 8, 16, 22, 340, 41440, 0, 0, 0, 2, 3, 1, 0)),
    ("separable_nph13", 391, 36, 65, 18, 4, 3, 0, 0, "SEPARABLE", (1, 25, 8, 13, 5, 8, 16, 22, 408, 47424, 0, 0, 0, 2, 3, 1, 0)),
    ("separable_nph15_th2", 479, 130, 65, 37, 4, 3, 0, 0, "SEPARABLE", (1, 30, 15, 15, 8, 2, 16, 19, 500, 47984, 0, 0, 0, 2, 19, 1, 0)),
    ("separable_ntv68", 300, 340, 100, 20, 4, 3, 0, 0, "SEPARABLE", (1, 12, 68, 6, 35, 1, 16, 68, 204, 90560, 0, 0, 0, 2, 20, 1, 0)),
    ("separable_ntv79_lanczos", 20, 250, 65, 19, 4, 3, 0, 0, "SEPARABLE", (2, 6, 79, 3, 40, 2, 16, 93, 32, 59776, 0, 0, 0, 2, 10, 1, 0)),
    ("separable_nph8_window_over_160k", 520, 400, 65, 13, 4, 2, 0, 0, "SEPARABLE", (0, 16, 62, 8, 32, 1, 16, 62, 524, 161952, 0, 0, 0, 2, 13, 1, 0)),
    ("separable_nph10_window_over_160k", 587, 400, 65, 15, 4, 2, 0, 0, "SEPARABLE", (0, 19, 54, 10, 28, 1, 16, 54, 592, 155776, 0, 0, 0, 2, 15, 1, 0)),
    ("generic_window_refused", 618, 250, 65, 19, 4, 3, 0, 0, "GENERIC", (1, 39, 53, 20, 27, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0)),
    ("generic_12to1", 780, 240, 65, 20, 4, 3, 0, 0, "GENERIC", (1, 48, 48, 24, 25, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0)),
    ("generic_misaligned", 100, 50, 67, 37, 4, 3, 0, 2, "GENERIC", (1, 6, 6, 3, 4, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0)),
    ("generic_psize1", 100, 50, 67, 37, 1, 3, 0, 0, "GENERIC", (1, 6, 6, 3, 4, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0)),
    ("generic_psize3", 100, 50, 67, 37, 3, 3, 0, 0, "GENERIC", (1, 6, 6, 3, 4, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0)),
    ("refused", 260, 100, 4, 40, 4, 3, 0, 0, "REFUSED", (1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0)),
]]
BY_NAME = {r.name: r for r in ROWS}

SEP2_NPH = (1, 2, 3, 4, 5, 6, 7, 8, 10, 12)
# a tap pair count k_sep2 has, at most 64 vertical taps, and still k_separable: k_sep2's window (even row pairs, + 2 rows) is over 160 KB even with one-row
# tiles while k_separable's, a little smaller, fits -- long vertical filters on wide windows, within 2 KB of the LDS limit
SEP2_WINDOW = "k_sep2 count, window over 160 KB"
# every (path, parameter) the planner can return.  SEP2P_MFMA: (K blocks, filter, ratio) -- one K block only at 2:1, two for every (filter, ratio) the window
# c0 + 3 r + nt <= 32 admits (test_matrix_core_admission sweeps r = 2..8 x the three filters for it)
REACHABLE = set(
    [("HALF8S", "bicubic"), ("HALF8S", "bilinear")] +
    [("SEP2", n) for n in SEP2_NPH] +
    [("SEP2P", n) for n in SEP2_NPH] +
    [("SEP2P_MFMA", 1, "bilinear", 2), ("SEP2P_MFMA", 1, "bicubic", 2)] +
    [("SEP2P_MFMA", 2, "bilinear", 3), ("SEP2P_MFMA", 2, "bilinear", 4), ("SEP2P_MFMA", 2, "bilinear", 5), ("SEP2P_MFMA", 2, "bilinear", 6),
     ("SEP2P_MFMA", 2, "bicubic", 3), ("SEP2P_MFMA", 2, "bicubic", 4), ("SEP2P_MFMA", 2, "lanczos", 2)] +
    [("SEPARABLE", "nph 9"), ("SEPARABLE", "nph 11"), ("SEPARABLE", "nph >= 13"), ("SEPARABLE", "ntv > 64"), ("SEPARABLE", SEP2_WINDOW)] +
    [("GENERIC", "psize 4, planner refusal"), ("GENERIC", "psize 4, misaligned"), ("GENERIC", "psize 1"), ("GENERIC", "psize 3")] +
    [("REFUSED",)])
# what the query proves unreachable, and was deleted from launch_sep for it
UNREACHABLE = [
    ("k_separable<8, 8>", "8 x 8 taps are 4 tap pairs: k_sep2<4> (or k_half8s) takes them; its window at one-row tiles is far below the 160 KB at which k_sep2 declines"),
    ("k_separable<5, 5>", "5 taps (the binomial blur's bank, bicubic below 1.25:1) are 3 tap pairs: k_sep2<3>"),
    ("k_separable<4, 4>", "4 taps (bilinear up to 2:1) are 2 tap pairs: k_sep2<2>"),
    ("k_separable<2, 2>", "2 taps (bilinear enlarging) are 1 tap pair: k_sep2<1>"),
    ("k_separable<6, 6>", "6 taps (lanczos enlarging, bicubic up to 1.5:1) are 3 tap pairs: k_sep2<3>"),
]
FILTERS = ("bilinear", "bicubic", "lanczos")


def pitches(r):
    return align(r.sw * r.psize, 16) + r.ipad, align(r.dw * r.psize, 16) + 16


def plan(r, ops, src_bits=0, dst_bits=0, ntracks=1, mode=lib.PLAN_RESIZE):
    irow, orow = pitches(r)
    return ops.resize_plan(r.sw, r.sh, r.dw, r.dh, r.psize, r.interp, irow=irow, orow=orow, src_bits=src_bits, dst_bits=dst_bits, ntracks=ntracks, mode=mode)


def key(d, psize=4, aligned=True):
    """the (path, parameter) pair of a plan: what REACHABLE lists"""
    p = d["path"]
    if p == "HALF8S":
        return (p, FILTERS[d["kernel"]])
    if p in ("SEP2", "SEP2P"):
        return (p, d["nph"])
    if p == "SEP2P_MFMA":
        return (p, d["mh_kb"], FILTERS[d["kernel"]], d["mh_r"])
    if p == "SEPARABLE":
        return (p, "ntv > 64" if d["ntv"] > 64 else "nph %d" % d["nph"] if d["nph"] in (9, 11) else "nph >= 13" if d["nph"] >= 13 else SEP2_WINDOW)
    if p == "GENERIC":
        return (p, "psize %d" % psize if psize != 4 else "psize 4, planner refusal" if aligned else "psize 4, misaligned")
    return (p,)


def row_key(r, d):
    irow, orow = pitches(r)
    return key(d, r.psize, (irow | orow) & 3 == 0)


def describe(r, d):
    return "%s: %dx%d -> %dx%d psize %d interp %d force %d pitch +%d, planned %s" % (r.name, r.sw, r.sh, r.dw, r.dh, r.psize, r.interp, r.force, r.ipad, row_key(r, d))


@pytest.fixture
def ops_cpu():
    """lives_amd.ops without a device: only its host-side calls (the plan query, the tuning table) are used"""
    from lives_amd import ops
    lib.load()
    return ops


# ------------------------------------------------------------------------------------------------------------------ CPU: the table against the planner
def test_every_row_takes_the_path_written_in_the_table(ops_cpu, tune):
    for r in ROWS:
        tune("SEP2P_FORCE", 1 if r.force else -1)
        d = plan(r, ops_cpu)
        assert d["path"] == r.path, describe(r, d)
        assert tuple(d[f] for f in PLAN_FIELDS) == r.plan, "%s: plan %s, table %s" % (describe(r, d), dict((f, d[f]) for f in PLAN_FIELDS), dict(zip(PLAN_FIELDS, r.plan)))
        assert (d["rc"] == 0) == (r.path != "REFUSED")


def test_the_table_covers_exactly_what_the_planner_can_return(ops_cpu, tune):
    got = set()
    for r in ROWS:
        tune("SEP2P_FORCE", 1 if r.force else -1)
        got.add(row_key(r, plan(r, ops_cpu)))
    assert got == REACHABLE, "rows without a listed path: %s; listed paths without a row: %s" % (sorted(got - REACHABLE, key=str), sorted(REACHABLE - got, key=str))


def test_rows_keep_to_the_shape_rules(ops_cpu, tune):
    """two tile columns with a partial last one; two tile rows of the launched height with a partial last one (one-row tiles cannot be partial); the filter windows of
    the first and the last output sample reach past the frame on both axes, so the clamp works at all four borders; nothing much larger than 800 x 400"""
    L = lib.load()
    halved, forced_low = set(), False
    for r in ROWS:
        tune("SEP2P_FORCE", 1 if r.force else -1)
        d = plan(r, ops_cpu)
        assert r.sw <= 800 and r.sh <= 400 and r.dw <= 800 and r.dh <= 400, r.name
        if r.path == "REFUSED":
            continue
        assert r.dw >= 65 and r.dw % 64, r.name
        if r.path != "GENERIC":
            assert d["tiles_x"] >= 2 and d["tiles_y"] >= 2 and (r.dh % d["th"] or d["th"] == 1), describe(r, d)
            if d["th"] < d["th_start"]:
                halved.add(r.path)
            forced_low |= r.path == "SEP2P" and r.force and d["th"] < 4
        for (srcn, dstn) in ((r.sw, r.dw), (r.sh, r.dh)):
            nt = ctypes.c_int()
            pos, co = np.zeros(dstn, np.int32), np.zeros(dstn * 256, np.int16)
            assert L.lgpu_make_filter(srcn, dstn, d["kernel"], ctypes.byref(nt), P(pos), P(co), 256) == 0
            assert pos[0] < 0 and pos[-1] + nt.value > srcn, "%s: %d -> %d is not clamped at both ends" % (r.name, srcn, dstn)
    assert halved == {"SEP2", "SEP2P", "SEP2P_MFMA", "SEPARABLE"}, "a row per family with the tile height halved by its LDS budget: %s" % sorted(halved)
    assert forced_low, "a forced k_sep2p row with tiles below 4 rows (which the default leaves to k_sep2)"


def test_matrix_core_admission(ops_cpu, tune):
    """k_sep2p<1, KB, 4>: which (filter, integer ratio) the planner admits -- r = 2..8 x the three filters, forced so that no tile-height rule hides an admission"""
    tune("SEP2P_FORCE", 1)
    got = set()
    for kernel, (interp, sh, dh) in enumerate([(2, 50, 37), (3, 50, 37), (3, 30, 75)]):
        for r in range(2, 9):
            d = ops_cpu.resize_plan(68 * r, sh, 68, dh, 4, interp)
            assert d["kernel"] == kernel and d["path"] in ("SEP2", "SEP2P", "SEP2P_MFMA", "SEPARABLE"), (kernel, r, d)
            if d["path"] == "SEP2P_MFMA":
                got.add(key(d))
    assert got == {k for k in REACHABLE if k[0] == "SEP2P_MFMA"}


def test_no_geometry_leaves_the_listed_paths(ops_cpu, tune):
    """a sweep of ratios, both byte alignments of the source width, the three filters, with and without SEP2P_FORCE: every plan is one of REACHABLE.  In
    particular k_separable is only ever asked for tap counts k_sep2 has no instantiation for, more than 64 vertical taps, or long vertical filters whose
    k_sep2 window passes 160 KB: never for the up to 8 x 8 taps of the five fixed k_separable<H, V> (UNREACHABLE), which had no caller and are gone"""
    assert len(UNREACHABLE) == 5
    seen = set()
    for force in (0, 1):
        tune("SEP2P_FORCE", 1 if force else -1)
        for interp in (2, 3):
            for dw in (65, 130):
                for sw in list(range(8, 800, 7)) + [dw, 2 * dw, 3 * dw, 4 * dw, 6 * dw]:
                    for (sh, dh) in ((36, 18), (50, 37), (30, 75), (330, 19), (37, 37), (200, 37), (250, 19), (400, 13), (400, 15), (400, 21)):
                        if (sw, sh) == (dw, dh):
                            continue
                        d = ops_cpu.resize_plan(sw, sh, dw, dh, 4, interp)
                        k = key(d)
                        assert k in REACHABLE, "%dx%d -> %dx%d interp %d force %d: %s" % (sw, sh, dw, dh, interp, force, k)
                        if k == ("SEPARABLE", SEP2_WINDOW):          # k_sep2 declines only when one-row tiles do not fit either; k_separable then barely fits
                            assert d["th"] == 1 and d["ntv"] > 32 and d["lds"] > 128 * 1024, (sw, sh, dw, dh, interp, d)
                        seen.add(k)
    assert {k[0] for k in seen} == {"HALF8S", "SEP2", "SEP2P", "SEP2P_MFMA", "SEPARABLE", "GENERIC"}
    assert {k for k in seen if k[0] == "SEPARABLE"} == {k for k in REACHABLE if k[0] == "SEPARABLE"}


def test_query_refuses_what_the_entry_points_refuse(ops_cpu):
    for kw in (dict(psize=2), dict(irow=8), dict(ntracks=2), dict(mode=7)):
        with pytest.raises(lib.LgpuError):
            ops_cpu.resize_plan(100, 50, 67, 37, **kw)
    for kw in (dict(psize=3), dict(src_bits=2), dict(dst_bits=1), dict(irow=402)):       # lgpu_chain_check's LGPU_E_BADARG
        d = ops_cpu.resize_plan(100, 50, 67, 37, mode=lib.PLAN_CHAIN, **kw)
        assert (d["path"], d["rc"]) == ("REFUSED", -2), kw
    with pytest.raises(lib.LgpuError):
        ops_cpu.resize_plan(64, 64, 64, 64, mode=lib.PLAN_CHAIN)
    # flag bits in interp: lgpu_resize compares the whole number (not BEST: bilinear), the chain masks them off
    assert ops_cpu.resize_plan(100, 50, 67, 37, interp=3 | 0x200)["kernel"] == 0
    assert ops_cpu.resize_plan(100, 50, 67, 37, interp=3 | 0x200, mode=lib.PLAN_CHAIN)["kernel"] == 1
    # the chain has no generic passes: what lgpu_resize hands to them, lgpu_chain refuses
    r = BY_NAME["generic_window_refused"]
    assert plan(r, ops_cpu)["path"] == "GENERIC"
    d = plan(r, ops_cpu, ntracks=3, mode=lib.PLAN_CHAIN)
    assert d["path"] == "REFUSED" and d["rc"] == -3


# ------------------------------------------------------------------------------------------------------------------ the table in docs/KERNELS.md
DOC_PATHS = [
    ("HALF8S", "`k_half8s`", "exact 2:1 on both axes, bicubic or bilinear, 4-byte aligned frames and pitches"),
    ("SEP2", "`k_sep2<nph>`", "`nph = ceil(nth / 2)` in {1..8, 10, 12}, at most 64 vertical taps, a window within 160 KB, and `k_sep2p` not taken"),
    ("SEP2P", "`k_sep2p<nph, 0, 4>`", "the same taps; `sw % 4 == 0`, 16-byte aligned source rows, a window within 48 x 64 DMA requests and 80 KB, at most 12 vertical tap "
     "pairs; shrinking launches of >= 1536 tiles with tiles of >= 4 rows (or `SEP2P_FORCE`)"),
    ("SEP2P_MFMA", "`k_sep2p<1, kb, 4>`", "as `k_sep2p`, and `sw % dw == 0`, ratio r >= 2, the same taps for every column, `c0 + 3 r + nt <= 32`; taken at any size "
     "when tiles have >= 4 rows"),
    ("SEPARABLE", "`k_separable<0, 0>`", "tap pair counts `k_sep2` has no instantiation for (9, 11, >= 13); more than 64 vertical taps; a `k_sep2` count whose `k_sep2` "
     "window passes 160 KB at one-row tiles while `k_separable`'s still fits (long vertical filters on wide windows)"),
    ("GENERIC", "`k_hpass_generic` + `k_vpass_generic`", "1- and 3-byte pixels; 4-byte pixels on frames or pitches that are not 4-byte aligned, or when no window fits "
     "160 KB of LDS"),
    ("REFUSED", "none", "more than 256 taps on an axis (`LGPU_E_UNSUPPORTED`, nothing written); in a chain also what `lgpu_resize` gives to the generic passes"),
]


def doc_table():
    """the path table of docs/KERNELS.md, generated from ROWS (python -c 'from tests import test_resize_plans as t; print(t.doc_table())')"""
    out = ["| path (`lgpu_debug_resize_plan`) | kernel | reached when | parameter: rows of `tests/test_resize_plans.py` (sw x sh -> dw x dh) |", "|---|---|---|---|"]
    for path, kernel, cond in DOC_PATHS:
        groups = {}
        for r in ROWS:
            if r.path == path:
                d = dict(zip(PLAN_FIELDS, r.plan), path=r.path)
                groups.setdefault(row_key(r, d)[1:], []).append((r, d))
        cells = []
        for k, rs in groups.items():
            label = "kb %d %s r %d" % k if path == "SEP2P_MFMA" else "nph %d" % k if path in ("SEP2", "SEP2P") else ", ".join(str(x) for x in k)
            cells.append((label + ": " if label else "") + ", ".join("`%s` (%dx%d -> %dx%d%s)" % (
                r.name, r.sw, r.sh, r.dw, r.dh, ", th %d of %d" % (d["th"], d["th_start"]) if d["th"] < d["th_start"] else "") for r, d in rs))
        out.append("| `%s` | %s | %s | %s |" % (path, kernel, cond, "; ".join(cells)))
    return "\n".join(out) + "\n"


def test_the_table_in_the_docs_is_the_one_generated_from_the_rows():
    import os
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "docs", "KERNELS.md")).read()
    assert doc_table() in text, "docs/KERNELS.md: replace the path table of the resize section with doc_table()'s output"


# ------------------------------------------------------------------------------------------------------------------ random geometry
Draw = namedtuple("Draw", "sw sh dw dh psize interp irow orow force")
_DRAWS = {}


def draws():
    """200 seeded resizes: sw 1..400, sh 1..200, destination sides from 1/24 of the source side (so that no filter exceeds 256 taps: lanczos 6 x 24 = 144) to
    500 x 260, every pixel size, both filters, pitch = row + 0 / 4 / 8 bytes.  Every third 4-byte draw has its source width rounded up to a multiple of 4 and
    16-byte pitches, and comes twice: as it is and under SEP2P_FORCE"""
    if "d" not in _DRAWS:
        rng = np.random.default_rng(0x5E92)
        out, n4 = [], 0
        for _ in range(200):
            sw, sh = int(rng.integers(1, 401)), int(rng.integers(1, 201))
            psize, interp = int(rng.choice([1, 3, 4])), int(rng.choice([2, 3]))
            pad_i, pad_o = int(rng.choice([0, 4, 8])), int(rng.choice([0, 4, 8]))
            fr = [float(rng.random()), float(rng.random())]
            twice = False
            if psize == 4:
                n4 += 1
                if n4 % 3 == 0:
                    sw, twice = align(sw, 4), True
            lo_w, lo_h = max(1, -(-sw // 24)), max(1, -(-sh // 24))
            dw, dh = lo_w + int(fr[0] * (500 - lo_w + 1)), lo_h + int(fr[1] * (260 - lo_h + 1))
            if (sw, sh) == (dw, dh):
                dh += 1
            irow, orow = sw * psize + pad_i, dw * psize + pad_o
            if twice:
                irow, orow = align(sw * 4, 16) + 4 * pad_i, align(dw * 4, 16) + 4 * pad_o
            out.append(Draw(sw, sh, dw, dh, psize, interp, irow, orow, 0))
            if twice:
                out.append(Draw(sw, sh, dw, dh, psize, interp, irow, orow, 1))
        _DRAWS["d"] = out
    return _DRAWS["d"]


_WANT = {}


def oracle_resize(orc, tag, sw, sh, dw, dh, psize, interp, irow, seed):
    """(source frame, the oracle's frame), computed once per case and shared by the tests of a session"""
    if tag not in _WANT:
        rng = np.random.default_rng(seed)
        src = rng.integers(0, 256, (sh, irow), dtype=np.uint8)
        want = np.zeros((dh, dw * psize), np.uint8)
        rc = orc.orc_resize(P(src), irow, sw, sh, P(want), dw * psize, dw, dh, psize, interp)
        want.setflags(write=False)
        _WANT[tag] = (src, want, rc)
    return _WANT[tag]


def draw_want(orc, i, dr):
    return oracle_resize(orc, ("draw", dr.sw, dr.sh, dr.dw, dr.dh, dr.psize, dr.interp, dr.irow), dr.sw, dr.sh, dr.dw, dr.dh, dr.psize, dr.interp, dr.irow, 7000 + i - dr.force)


def test_random_draws_are_all_served(orc, ops_cpu, tune):
    """the seed's 200 draws: none is skipped -- the oracle resizes every one, the planner refuses none -- and they spread over the paths"""
    ds = draws()
    assert sum(1 for d in ds if not d.force) == 200 and sum(1 for d in ds if d.force) >= 15
    paths = {}
    for i, dr in enumerate(ds):
        assert 1 <= dr.sw <= 400 and 1 <= dr.sh <= 200 and dr.dw <= 500 and dr.dh <= 260 and dr.sw <= 24 * dr.dw and dr.sh <= 24 * dr.dh, dr
        assert draw_want(orc, i, dr)[2] == 0, dr
        tune("SEP2P_FORCE", 1 if dr.force else -1)
        d = ops_cpu.resize_plan(dr.sw, dr.sh, dr.dw, dr.dh, dr.psize, dr.interp, irow=dr.irow, orow=dr.orow)
        assert d["path"] != "REFUSED", dr
        paths[d["path"]] = paths.get(d["path"], 0) + 1
    print("paths of the draws:", paths)
    assert {"SEP2", "SEP2P", "SEPARABLE", "GENERIC"} <= set(paths), paths


# ------------------------------------------------------------------------------------------------------------------ GPU
FILL = 0xA5


def gpu_resize(gpu, src, sw, sh, dw, dh, psize, interp, orow, what):
    """lgpu_resize into a 0xA5-filled destination with a guard row; returns (frame bytes, plan with the real pointers).  The guard row and the row padding
    must keep their fill"""
    d_src = dev(src)
    d_dst = dev(np.full((dh + 1, orow), FILL, np.uint8))
    d = gpu.resize_plan(sw, sh, dw, dh, psize, interp, irow=src.strides[0], orow=orow, src_bits=d_src.data_ptr(), dst_bits=d_dst.data_ptr())
    gpu.resize(d_src, d_dst, sw, sh, dw, dh, psize=psize, interp=interp)
    out = host(d_dst)
    assert (out[dh] == FILL).all(), "%s (%s): the row past the frame was written" % (what, d["path"])
    assert (out[:dh, dw * psize:] == FILL).all(), "%s (%s): row padding was written" % (what, d["path"])
    return out[:dh, :dw * psize], d


def same_bytes(got, want, what):
    bad = got != want
    assert not bad.any(), "%s: %d bytes differ from the oracle, first at (row, byte) %s: got %d, want %d" % (
        what, int(bad.sum()), np.argwhere(bad)[0].tolist(), got[tuple(np.argwhere(bad)[0])], want[tuple(np.argwhere(bad)[0])])


@gpu_mark
@pytest.mark.parametrize("r", ROWS, ids=lambda r: r.name)
def test_row_equals_the_oracle_on_its_kernel(gpu, orc, tune, r):
    tune("SEP2P_FORCE", 1 if r.force else -1)
    irow, orow = pitches(r)
    if r.path == "REFUSED":
        src = np.random.default_rng(1).integers(0, 256, (r.sh, irow), dtype=np.uint8)
        d_src, d_dst = dev(src), dev(np.full((r.dh + 1, orow), FILL, np.uint8))
        assert plan(r, gpu, d_src.data_ptr(), d_dst.data_ptr())["path"] == "REFUSED"
        with pytest.raises(lib.LgpuError):
            gpu.resize(d_src, d_dst, r.sw, r.sh, r.dw, r.dh, psize=r.psize, interp=r.interp)
        assert (host(d_dst) == FILL).all(), "a refused resize wrote to its destination"
        return
    src, want, rc = oracle_resize(orc, ("row", r.name), r.sw, r.sh, r.dw, r.dh, r.psize, r.interp, irow, 6000 + ROWS.index(r))
    assert rc == 0
    got, d = gpu_resize(gpu, src, r.sw, r.sh, r.dw, r.dh, r.psize, r.interp, orow, r.name)
    assert d["path"] == r.path and tuple(d[f] for f in PLAN_FIELDS) == r.plan, describe(r, d)
    same_bytes(got, want, describe(r, d))


# one row per (path, nph / K blocks) a chain can reach (the chain takes 4-byte frames and has no generic passes)
CHAIN_ROWS = ["half8s_bicubic", "half8s_bilinear", "sep2_1", "sep2_2", "sep2_3", "sep2_4", "sep2_5_halved", "sep2_6", "sep2_7", "sep2_8", "sep2_10", "sep2_12_lanczos",
              "sep2p_1", "sep2p_2", "sep2p_3", "sep2p_4", "sep2p_5_halved", "sep2p_6_lanczos", "sep2p_7", "sep2p_8", "sep2p_10_th2", "sep2p_12",
              "mfma_kb1_bilinear", "mfma_kb1_bicubic", "mfma_kb2_bilinear_r5", "mfma_kb2_bicubic_r3", "mfma_kb2_lanczos_r2",
              "separable_nph9", "separable_nph11", "separable_nph13", "separable_ntv79_lanczos", "separable_nph8_window_over_160k"]


def test_chain_rows_cover_every_path_a_chain_reaches():
    keys = {REACH[:2] for REACH in (row_key(BY_NAME[n], dict(zip(PLAN_FIELDS, BY_NAME[n].plan), path=BY_NAME[n].path)) for n in CHAIN_ROWS)}
    assert keys == {k[:2] for k in REACHABLE if k[0] not in ("GENERIC", "REFUSED")}


def layer2(rng, dw, dh, irow2):
    """a second layer that is translucent, opaque and fully transparent in about equal parts"""
    a = rng.integers(0, 256, (dh, irow2), dtype=np.uint8)
    al = a[:, 3:dw * 4:4]
    kind = rng.integers(0, 3, al.shape)
    al[kind == 1] = 255
    al[kind == 2] = 0
    return a


def run_chain(gpu, orc, r, do_blur, seed):
    rng = np.random.default_rng(seed)
    ntr = 3
    irow, orow = pitches(r)
    irow2 = align(r.dw * 4, 16) + 32
    bf = int(rng.integers(1, 255))
    lut = rng.integers(0, 256, 256, dtype=np.uint8)
    srcs = [rng.integers(0, 256, (r.sh, irow), dtype=np.uint8) for _ in range(ntr)]
    l2s = [layer2(rng, r.dw, r.dh, irow2) for _ in range(ntr)]
    d_src, d_l2 = [dev(a) for a in srcs], [dev(a) for a in l2s]
    d_dst = [dev(np.full((r.dh + 1, orow), FILL, np.uint8)) for _ in range(ntr)]
    bits = lambda ts: int(np.bitwise_or.reduce([t.data_ptr() & 15 for t in ts]))
    d = plan(r, gpu, bits(d_src), bits(d_dst) | bits(d_l2), ntracks=ntr, mode=lib.PLAN_CHAIN_BLUR if do_blur else lib.PLAN_CHAIN)
    what = "chain blur=%d bf=%d, %s" % (do_blur, bf, describe(r, d))
    assert d["path"] == r.path, what
    prm = gpu.chain_params(r.sw, r.sh, irow, r.dw, r.dh, irow2, orow, swap_rb=1, interp=r.interp, do_blur=do_blur, bf=bf, lut=lut)
    gpu.chain(prm, gpu.chain_tracks(d_src, d_l2, d_dst))
    for i in range(ntr):
        want = np.zeros((r.dh, r.dw * 4), np.uint8)
        assert orc.orc_chain(P(srcs[i]), irow, r.sw, r.sh, P(l2s[i]), irow2, P(want), r.dw * 4, r.dw, r.dh, 1, r.interp, do_blur, bf, P(lut)) == 0
        out = host(d_dst[i])
        same_bytes(out[:r.dh, :r.dw * 4], want, "%s, track %d" % (what, i))
        assert (out[r.dh] == FILL).all() and (out[:r.dh, r.dw * 4:] == FILL).all(), "%s, track %d: bytes outside the frame were written" % (what, i)


@gpu_mark
@pytest.mark.parametrize("name", CHAIN_ROWS)
def test_chain_equals_the_oracle_on_every_kernel(gpu, orc, tune, name):
    """lgpu_chain (polyphase): three tracks, R <-> B swap (src_sel, and the B fragment of the matrix-core pass), a blend amount strictly inside 0..255, a random
    LUT, a layer 2 that is partly translucent, partly opaque, partly transparent: each track equals orc_chain byte for byte"""
    r = BY_NAME[name]
    tune("SEP2P_FORCE", 1 if r.force else -1)
    run_chain(gpu, orc, r, 0, 8000 + CHAIN_ROWS.index(name))


@gpu_mark
def test_blur_chain_with_a_k_sep2_resize_stage(gpu, orc, tune):
    """do_blur: the resize stage writes compact intermediate frames; here through k_sep2<5> at 2.26:1 x 3.5:1 with halved tiles"""
    tune("SEP2P_FORCE", -1)
    run_chain(gpu, orc, BY_NAME["sep2_5_halved"], 1, 8100)


@gpu_mark
def test_chain_refuses_a_window_no_kernel_holds(gpu, tune):
    """what lgpu_resize gives to its generic passes the chain refuses (it has none), before anything is written"""
    tune("SEP2P_FORCE", -1)
    r = BY_NAME["generic_window_refused"]
    irow, orow = pitches(r)
    rng = np.random.default_rng(8200)
    d_src = [dev(rng.integers(0, 256, (r.sh, irow), dtype=np.uint8))]
    d_l2 = [dev(layer2(rng, r.dw, r.dh, orow))]
    d_dst = [dev(np.full((r.dh + 1, orow), FILL, np.uint8))]
    assert plan(r, gpu, mode=lib.PLAN_CHAIN)["path"] == "REFUSED"
    prm = gpu.chain_params(r.sw, r.sh, irow, r.dw, r.dh, orow, orow, swap_rb=1, interp=r.interp, do_blur=0, bf=100, lut=None)
    with pytest.raises(lib.LgpuError):
        gpu.chain(prm, gpu.chain_tracks(d_src, d_l2, d_dst))
    assert (host(d_dst[0]) == FILL).all()


@gpu_mark
def test_random_geometry_equals_the_oracle(gpu, orc, tune):
    """the draws of draws(): every one byte for byte, none skipped; the failure message carries the geometry and the path the planner took"""
    n = 0
    for i, dr in enumerate(draws()):
        src, want, rc = draw_want(orc, i, dr)
        assert rc == 0, dr
        tune("SEP2P_FORCE", 1 if dr.force else -1)
        got, d = gpu_resize(gpu, src, dr.sw, dr.sh, dr.dw, dr.dh, dr.psize, dr.interp, dr.orow, str(dr))
        same_bytes(got, want, "draw %d %s, planned %s" % (i, dr, key(d, dr.psize, (dr.irow | dr.orow) & 3 == 0)))
        n += 1
    assert n == len(draws()) and n >= 215
