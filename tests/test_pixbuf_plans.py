"""The gdk-pixbuf scaler (lgpu_pixbuf_scale, lgpu_pixbuf_scale_batch, the fused chain's scale) on every kernel its dispatcher can choose.

pixbuf.hip's pb_plan picks one of more than a hundred template instantiations per call -- k_pb_nearest, k_pb_double, k_pb_half3, k_pb_half, k_pb_up<NP, NY>,
k_pb_gather<NP>, k_pb_pairs<CH, NP, NY, PRE> in two tile orders, k_pb_window<CH, UNIFORM>, k_pb_direct<CH>, a plain copy, a refusal, PB_NOT_FUSED for the chain --
from the tap box of the geometry's weight table, a 16-bit test on the weights, integer steps, alignment, two LDS budgets and two tuning switches.
lgpu_debug_pixbuf_plan answers, on the host and through the very function the launch switches on, which one a call takes.  ROWS is a table of small geometries with
the plan each is expected to take; a key is the family with its template arguments, for k_pb_pairs also the tile order (OPQ and PbEpi are run per row, below):

  CPU  every row's plan is the one written here, field by field; the keys of the table are exactly REACHABLE (written out below), and so are the keys a sweep of
       the query over a finite family returns, so deleting a row, adding an arm or an arm going dead fails; the rows keep to the shape rules; the table in
       docs/KERNELS.md is the one generated from the rows
  GPU  every row: the plan with the real pointers, then lgpu_pixbuf_scale == orc_pixbuf_scale byte for byte with three alpha mixes, guard row and row padding
       untouched; the OPQ form of every row that has one; the PbEpi form of every row that has one through lgpu_chain_amounts (three tracks, R <-> B, amounts, a
       LUT) against the oracle's stages and against the staged path, and again with LGPU_INTERP_OPAQUE (OPQ x PbEpi); one row per family through
       lgpu_pixbuf_scale_batch with a misaligned frame, the exact-ratio families also all aligned; 200 random geometries

The arithmetic is integer-exact: no tolerance anywhere.
"""
import os
from collections import namedtuple

import numpy as np
import pytest

from lives_amd import lib
from oracle import pyoracle as po
from tests import chain_ref
from tests.util import align, dev, host

P = po.P
gpu_mark = pytest.mark.gpu
PIXBUF, OPAQUE = 0x100, 0x200

Row = namedtuple("Row", "name sw sh dw dh ch interp tune path plan")
PLAN_FIELDS = ("ch", "np", "ny", "pre", "opq", "epi", "hyper", "aligned", "uniform", "tile_h", "win_h", "win_w", "lds", "gx", "gy", "gz", "tiles_x", "tiles_y", "per_xcd",
               "strips", "cgroups", "bands", "rb", "x_step", "y_step", "tx0", "tx1", "ty0", "ty1", "n_x", "n_y", "nq", "rnd")

# name, sw, sh, dw, dh, channels, interp, tuning switch ("NAME=value" or ""), path, PLAN_FIELDS.  Source rows: sw * channels rounded up to 16 bytes; destination
# rows: dw * channels rounded up to 16 + 16 bytes of padding; frames 16-byte aligned (pitches()).  The plans were taken from the query (rows_source()).  A
# NOT_FUSED row is asked in chain mode; every other row as a plain scale.  *_small: dw < 64, every wave ends inside the frame; *_narrow: the source is narrower
# than the used tap row, so every tap row clamps at both ends at once.  The wide k_pb_direct rows need a window over 48 KB: long and thin; its narrow rows a
# window no budget holds at few pixels: 30 x 27 -> 1 x 1 HYPER has 33 x 30 taps, of which 32 lie on a 30-pixel row.
ROWS = [Row(*r) for r in [
    ("direct3", 1820, 32, 65, 9, 3, 3, "", "DIRECT", (3, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1795, 0, 2, 3, 1, 0, 0, 0, 0, 0, 0, 0, 1835008, 233016, 0, 31, 0, 7, 31, 7, 0, 0xffff)),
    ("direct4", 1820, 32, 65, 9, 4, 3, "", "DIRECT", (4, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1795, 0, 2, 3, 1, 0, 0, 0, 0, 0, 0, 0, 1835008, 233016, 0, 31, 0, 7, 31, 7, 0, 0xffff)),
    ("double", 100, 19, 200, 38, 4, 2, "", "DOUBLE", (0, 0, 0, 0, 0, 0, 0, 0, 0, 3, 0, 0, 0, 8, 1, 1, 0, 0, 0, 1, 1, 7, 0, 32768, 32768, 0, 2, 0, 2, 2, 2, 0, 0xffff)),
    ("gather_1", 65, 27, 65, 9, 4, 2, "", "GATHER", (0, 1, 0, 0, 0, 0, 0, 0, 0, 4, 0, 0, 0, 2, 3, 1, 0, 0, 0, 0, 0, 0, 0, 65536, 196608, 0, 2, 0, 4, 2, 4, 0, 0xffff)),
    ("gather_2", 65, 18, 65, 9, 4, 3, "", "GATHER", (0, 2, 0, 0, 0, 0, 0, 0, 0, 4, 0, 0, 0, 2, 3, 1, 0, 0, 0, 0, 0, 0, 0, 65536, 131072, 0, 3, 0, 4, 4, 5, 0, 0xffff)),
    ("gather_3", 195, 9, 65, 9, 4, 3, "", "GATHER", (0, 3, 0, 0, 0, 0, 0, 0, 0, 4, 0, 0, 0, 2, 3, 1, 0, 0, 0, 0, 0, 0, 0, 196608, 65536, 0, 6, 0, 4, 6, 4, 0, 0xffff)),
    ("gather_4", 325, 9, 65, 9, 4, 3, "", "GATHER", (0, 4, 0, 0, 0, 0, 0, 0, 0, 4, 0, 0, 0, 2, 3, 1, 0, 0, 0, 0, 0, 0, 0, 327680, 65536, 0, 7, 0, 3, 8, 4, 0, 0xffff)),
    ("half_bilinear", 140, 18, 70, 9, 4, 2, "", "HALF", (0, 0, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 131072, 131072, 0, 2, 0, 2, 3, 3, 0, 0xffff)),
    ("half_hyper", 140, 18, 70, 9, 4, 3, "", "HALF", (0, 0, 0, 0, 0, 0, 1, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 131072, 131072, 0, 4, 0, 4, 5, 5, 0, 0xffff)),
    ("half3_bilinear", 400, 18, 200, 9, 3, 2, "", "HALF3", (0, 0, 0, 0, 0, 0, 0, 0, 0, 6, 0, 0, 0, 8, 1, 1, 0, 0, 0, 2, 1, 2, 0, 131072, 131072, 0, 2, 0, 2, 3, 3, 0, 0xffff)),
    ("half3_hyper", 400, 18, 200, 9, 3, 3, "", "HALF3", (0, 0, 0, 0, 0, 0, 1, 0, 0, 6, 0, 0, 0, 8, 1, 1, 0, 0, 0, 2, 1, 2, 0, 131072, 131072, 0, 4, 0, 4, 5, 5, 0, 0xffff)),
    ("nearest3", 26, 14, 65, 9, 3, 0, "", "NEAREST", (3, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 2, 3, 1, 0, 0, 0, 0, 0, 0, 0, 26214, 101944, 0, 0, 0, 0, 0, 0, 0, 0x0)),
    ("nearest4", 26, 14, 65, 9, 4, 0, "", "NEAREST", (4, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 2, 3, 1, 0, 0, 0, 0, 0, 0, 0, 26214, 101944, 0, 0, 0, 0, 0, 0, 0, 0x0)),
    ("pairs3_00", 292, 8, 65, 9, 3, 3, "", "PAIRS", (3, 0, 0, 0, 0, 0, 0, 0, 0, 4, 8, 156, 19968, 2, 3, 1, 2, 3, 0, 0, 0, 0, 0, 294407, 58254, 0, 8, 0, 4, 8, 4, 2, 0xffff)),
    ("pairs3_00_xcd", 455, 30, 65, 75, 3, 3, "", "PAIRS", (3, 0, 0, 0, 0, 0, 0, 0, 0, 2, 6, 232, 22272, 80, 1, 1, 2, 38, 10, 0, 0, 0, 0, 458752, 26214, 0, 10, 0, 4, 10, 4, 2, 0xffff)),
    ("pairs3_10", 65, 9, 65, 18, 3, 2, "", "PAIRS", (3, 1, 0, 0, 0, 0, 0, 0, 0, 16, 11, 40, 7040, 2, 2, 1, 2, 2, 0, 0, 0, 0, 0, 65536, 32768, 0, 1, 0, 2, 2, 2, 1, 0x8000)),
    ("pairs3_10_xcd", 65, 750, 65, 75, 3, 2, "", "PAIRS", (3, 1, 0, 0, 0, 0, 0, 0, 0, 2, 21, 40, 13440, 80, 1, 1, 2, 38, 10, 0, 0, 0, 0, 65536, 655360, 0, 1, 0, 10, 2, 11, 1, 0xffff)),
    ("pairs3_20", 8, 72, 70, 9, 3, 3, "", "PAIRS", (3, 2, 0, 0, 0, 0, 0, 0, 0, 8, 67, 12, 12864, 2, 2, 1, 2, 2, 0, 0, 0, 0, 0, 7489, 524288, 0, 3, 0, 10, 4, 11, 1, 0xffff)),
    ("pairs3_20_xcd", 8, 2400, 70, 150, 3, 3, "", "PAIRS", (3, 2, 0, 0, 0, 0, 0, 0, 0, 4, 67, 12, 12864, 80, 1, 1, 2, 38, 10, 0, 0, 0, 0, 7489, 1048576, 0, 3, 0, 18, 4, 19, 1, 0xffff)),
    ("pairs3_22", 16, 9, 65, 18, 3, 2, "", "PAIRS", (3, 2, 2, 0, 0, 0, 0, 0, 0, 16, 11, 16, 2816, 2, 2, 1, 2, 2, 0, 0, 0, 0, 0, 16131, 32768, 0, 2, 0, 2, 2, 2, 1, 0x8000)),
    ("pairs3_22_xcd", 50, 33, 200, 301, 3, 2, "", "PAIRS", (3, 2, 2, 0, 0, 0, 0, 0, 0, 16, 5, 16, 1280, 80, 1, 1, 4, 19, 10, 0, 0, 0, 0, 16384, 7185, 0, 2, 0, 2, 2, 2, 1, 0x8000)),
    ("pairs3_22_pre", 195, 18, 65, 9, 3, 2, "", "PAIRS", (3, 2, 2, 1, 0, 0, 0, 0, 0, 4, 9, 104, 14976, 2, 3, 1, 2, 3, 0, 0, 0, 0, 0, 196608, 131072, 0, 3, 0, 2, 4, 3, 1, 0xffff)),
    ("pairs3_22_pre_xcd", 195, 300, 65, 150, 3, 2, "", "PAIRS", (3, 2, 2, 1, 0, 0, 0, 0, 0, 4, 9, 104, 14976, 80, 1, 1, 2, 38, 10, 0, 0, 0, 0, 196608, 131072, 0, 3, 0, 2, 4, 3, 1, 0xffff)),
    ("pairs3_23", 16, 9, 65, 18, 3, 3, "", "PAIRS", (3, 2, 3, 0, 0, 0, 0, 0, 0, 16, 12, 16, 3072, 2, 2, 1, 2, 2, 0, 0, 0, 0, 0, 16131, 32768, 0, 3, 0, 3, 4, 4, 1, 0xffff)),
    ("pairs3_23_xcd", 50, 33, 200, 301, 3, 3, "", "PAIRS", (3, 2, 3, 0, 0, 0, 0, 0, 0, 16, 6, 16, 1536, 80, 1, 1, 4, 19, 10, 0, 0, 0, 0, 16384, 7185, 0, 3, 0, 3, 4, 4, 1, 0xffff)),
    ("pairs3_23_pre", 130, 27, 65, 9, 3, 2, "", "PAIRS", (3, 2, 3, 1, 0, 0, 0, 0, 0, 4, 13, 72, 14976, 2, 3, 1, 2, 3, 0, 0, 0, 0, 0, 131072, 196608, 0, 2, 0, 3, 3, 4, 1, 0xffff)),
    ("pairs3_23_pre_xcd", 130, 375, 65, 150, 3, 2, "", "PAIRS", (3, 2, 3, 1, 0, 0, 0, 0, 0, 4, 12, 72, 13824, 80, 1, 1, 2, 38, 10, 0, 0, 0, 0, 131072, 163840, 0, 2, 0, 3, 3, 4, 1, 0xffff)),
    ("pairs3_30", 8, 90, 70, 9, 3, 3, "", "PAIRS", (3, 3, 0, 0, 0, 0, 0, 0, 0, 8, 84, 12, 16128, 2, 2, 1, 2, 2, 0, 0, 0, 0, 0, 7489, 655360, 0, 4, 0, 13, 4, 13, 1, 0xffff)),
    ("pairs3_30_xcd", 8, 3000, 70, 150, 3, 3, "", "PAIRS", (3, 3, 0, 0, 0, 0, 0, 0, 0, 4, 84, 12, 16128, 80, 1, 1, 2, 38, 10, 0, 0, 0, 0, 7489, 1310720, 0, 4, 0, 23, 4, 23, 1, 0xffff)),
    ("pairs3_33", 54, 9, 65, 18, 3, 3, "", "PAIRS", (3, 3, 3, 0, 0, 0, 0, 0, 0, 16, 12, 36, 6912, 2, 2, 1, 2, 2, 0, 0, 0, 0, 0, 54445, 32768, 0, 4, 0, 3, 4, 4, 1, 0xffff)),
    ("pairs3_33_xcd", 400, 33, 200, 301, 3, 3, "", "PAIRS", (3, 3, 3, 0, 0, 0, 0, 0, 0, 16, 6, 72, 6912, 80, 1, 1, 4, 19, 10, 0, 0, 0, 0, 131072, 7185, 0, 4, 0, 3, 5, 4, 1, 0xffff)),
    ("pairs3_33_pre", 228, 11, 65, 9, 3, 2, "", "PAIRS", (3, 3, 3, 1, 0, 0, 0, 0, 0, 4, 8, 120, 15360, 2, 3, 1, 2, 3, 0, 0, 0, 0, 0, 229880, 80099, 0, 5, 0, 3, 5, 3, 1, 0xffff)),
    ("pairs3_33_pre_xcd", 228, 180, 65, 150, 3, 2, "", "PAIRS", (3, 3, 3, 1, 0, 0, 0, 0, 0, 4, 8, 120, 15360, 80, 1, 1, 2, 38, 10, 0, 0, 0, 0, 229880, 78643, 0, 5, 0, 3, 5, 3, 1, 0xffff)),
    ("pairs3_34", 8, 12, 70, 18, 3, 3, "", "PAIRS", (3, 3, 4, 0, 0, 0, 0, 0, 0, 16, 15, 12, 2880, 2, 2, 1, 2, 2, 0, 0, 0, 0, 0, 7489, 43690, 0, 4, 0, 4, 4, 4, 1, 0xffff)),
    ("pairs3_34_xcd", 22, 33, 200, 301, 3, 3, "", "PAIRS", (3, 3, 4, 0, 0, 0, 0, 0, 0, 16, 7, 12, 1344, 80, 1, 1, 4, 19, 10, 0, 0, 0, 0, 7208, 7185, 0, 4, 0, 4, 4, 4, 1, 0xffff)),
    ("pairs3_34_pre", 175, 18, 70, 9, 3, 3, "", "PAIRS", (3, 3, 4, 1, 0, 0, 0, 0, 0, 4, 11, 88, 15488, 2, 3, 1, 2, 3, 0, 0, 0, 0, 0, 163840, 131072, 0, 5, 0, 4, 6, 5, 1, 0xffff)),
    ("pairs3_34_pre_xcd", 195, 225, 65, 150, 3, 3, "", "PAIRS", (3, 3, 4, 1, 0, 0, 0, 0, 0, 4, 10, 104, 16640, 80, 1, 1, 2, 38, 10, 0, 0, 0, 0, 196608, 98304, 0, 5, 0, 4, 6, 5, 1, 0xffff)),
    ("pairs3_35", 8, 22, 70, 18, 3, 3, "", "PAIRS", (3, 3, 5, 0, 0, 0, 0, 0, 0, 16, 25, 12, 4800, 2, 2, 1, 2, 2, 0, 0, 0, 0, 0, 7489, 80099, 0, 4, 0, 5, 4, 5, 1, 0xffff)),
    ("pairs3_35_xcd", 130, 304, 65, 301, 3, 3, "", "PAIRS", (3, 3, 5, 0, 0, 0, 0, 0, 0, 8, 14, 72, 16128, 80, 1, 1, 2, 38, 10, 0, 0, 0, 0, 131072, 66189, 0, 5, 0, 5, 5, 5, 1, 0xffff)),
    ("pairs3_35_pre", 130, 27, 65, 9, 3, 3, "", "PAIRS", (3, 3, 5, 1, 0, 0, 0, 0, 0, 4, 15, 72, 17280, 2, 3, 1, 2, 3, 0, 0, 0, 0, 0, 131072, 196608, 0, 4, 0, 5, 5, 6, 1, 0xffff)),
    ("pairs3_35_pre_xcd", 130, 375, 65, 150, 3, 3, "", "PAIRS", (3, 3, 5, 1, 0, 0, 0, 0, 0, 4, 14, 72, 16128, 80, 1, 1, 2, 38, 10, 0, 0, 0, 0, 131072, 163840, 0, 4, 0, 5, 5, 6, 1, 0xffff)),
    ("pairs3_40", 162, 8, 65, 9, 3, 3, "", "PAIRS", (3, 4, 0, 0, 0, 0, 0, 0, 0, 8, 12, 88, 16896, 2, 2, 1, 2, 2, 0, 0, 0, 0, 0, 163335, 58254, 0, 6, 0, 4, 6, 4, 1, 0xffff)),
    ("pairs3_40_xcd", 260, 128, 65, 75, 3, 3, "", "PAIRS", (3, 4, 0, 0, 0, 0, 0, 0, 0, 2, 8, 136, 17408, 80, 1, 1, 2, 38, 10, 0, 0, 0, 0, 262144, 111848, 0, 6, 0, 5, 7, 5, 1, 0xffff)),
    ("pairs3_46_pre", 136, 19, 65, 9, 3, 3, "", "PAIRS", (3, 4, 6, 1, 0, 0, 0, 0, 0, 4, 14, 76, 17024, 2, 3, 1, 2, 3, 0, 0, 0, 0, 0, 137121, 138353, 0, 6, 0, 6, 6, 6, 1, 0xffff)),
    ("pairs3_46_pre_xcd", 228, 158, 65, 75, 3, 3, "", "PAIRS", (3, 4, 6, 1, 0, 0, 0, 0, 0, 2, 10, 120, 19200, 80, 1, 1, 2, 38, 10, 0, 0, 0, 0, 229880, 138062, 0, 7, 0, 6, 7, 6, 1, 0xffff)),
    ("pairs4_00", 292, 8, 65, 9, 4, 3, "", "PAIRS", (4, 0, 0, 0, 0, 0, 0, 0, 0, 4, 8, 156, 19968, 2, 3, 1, 2, 3, 0, 0, 0, 0, 0, 294407, 58254, 0, 8, 0, 4, 8, 4, 2, 0xffff)),
    ("pairs4_00_xcd", 455, 30, 65, 75, 4, 3, "", "PAIRS", (4, 0, 0, 0, 0, 0, 0, 0, 0, 2, 6, 232, 22272, 80, 1, 1, 2, 38, 10, 0, 0, 0, 0, 458752, 26214, 0, 10, 0, 4, 10, 4, 2, 0xffff)),
    ("pairs4_10", 65, 32, 65, 9, 4, 2, "", "PAIRS", (4, 1, 0, 0, 0, 0, 0, 0, 0, 8, 31, 40, 19840, 2, 2, 1, 2, 2, 0, 0, 0, 0, 0, 65536, 233016, 0, 1, 0, 5, 2, 5, 1, 0xffff)),
    ("pairs4_10_xcd", 65, 825, 65, 150, 4, 2, "", "PAIRS", (4, 1, 0, 0, 0, 0, 0, 0, 0, 4, 24, 40, 15360, 80, 1, 1, 2, 38, 10, 0, 0, 0, 0, 65536, 360448, 0, 1, 0, 6, 2, 7, 1, 0xffff)),
    ("pairs4_20", 8, 72, 70, 9, 4, 3, "", "PAIRS", (4, 2, 0, 0, 0, 0, 0, 0, 0, 8, 67, 12, 12864, 2, 2, 1, 2, 2, 0, 0, 0, 0, 0, 7489, 524288, 0, 3, 0, 10, 4, 11, 1, 0xffff)),
    ("pairs4_20_xcd", 8, 2400, 70, 150, 4, 3, "", "PAIRS", (4, 2, 0, 0, 0, 0, 0, 0, 0, 4, 67, 12, 12864, 80, 1, 1, 2, 38, 10, 0, 0, 0, 0, 7489, 1048576, 0, 3, 0, 18, 4, 19, 1, 0xffff)),
    ("pairs4_22", 78, 8, 65, 19, 4, 2, "", "PAIRS", (4, 2, 2, 0, 0, 0, 0, 0, 0, 16, 10, 48, 7680, 2, 2, 1, 2, 2, 0, 0, 0, 0, 0, 78643, 27594, 0, 3, 0, 2, 3, 2, 1, 0xffff)),
    ("pairs4_22_xcd", 240, 33, 200, 301, 4, 2, "", "PAIRS", (4, 2, 2, 0, 0, 0, 0, 0, 0, 16, 5, 48, 3840, 80, 1, 1, 4, 19, 10, 0, 0, 0, 0, 78643, 7185, 0, 3, 0, 2, 3, 2, 1, 0xffff)),
    ("pairs4_23", 8, 22, 70, 18, 4, 2, "", "PAIRS", (4, 2, 3, 0, 0, 0, 0, 0, 0, 16, 23, 12, 4416, 2, 2, 1, 2, 2, 0, 0, 0, 0, 0, 7489, 80099, 0, 2, 0, 3, 2, 3, 1, 0xffff)),
    ("pairs4_23_xcd", 78, 572, 65, 301, 4, 2, "", "PAIRS", (4, 2, 3, 0, 0, 0, 0, 0, 0, 8, 18, 48, 13824, 80, 1, 1, 2, 38, 10, 0, 0, 0, 0, 78643, 124540, 0, 3, 0, 3, 3, 3, 1, 0xffff)),
    ("pairs4_23_pre", 130, 45, 65, 18, 4, 2, "", "PAIRS", (4, 2, 3, 1, 0, 0, 0, 0, 0, 4, 12, 72, 13824, 2, 5, 1, 2, 5, 0, 0, 0, 0, 0, 131072, 163840, 0, 2, 0, 3, 3, 4, 1, 0xffff)),
    ("pairs4_23_pre_xcd", 130, 375, 65, 150, 4, 2, "", "PAIRS", (4, 2, 3, 1, 0, 0, 0, 0, 0, 4, 12, 72, 13824, 80, 1, 1, 2, 38, 10, 0, 0, 0, 0, 131072, 163840, 0, 2, 0, 3, 3, 4, 1, 0xffff)),
    ("pairs4_30", 8, 90, 70, 9, 4, 3, "", "PAIRS", (4, 3, 0, 0, 0, 0, 0, 0, 0, 8, 84, 12, 16128, 2, 2, 1, 2, 2, 0, 0, 0, 0, 0, 7489, 655360, 0, 4, 0, 13, 4, 13, 1, 0xffff)),
    ("pairs4_30_xcd", 8, 3000, 70, 150, 4, 3, "", "PAIRS", (4, 3, 0, 0, 0, 0, 0, 0, 0, 4, 84, 12, 16128, 80, 1, 1, 2, 38, 10, 0, 0, 0, 0, 7489, 1310720, 0, 4, 0, 23, 4, 23, 1, 0xffff)),
    ("pairs4_33", 78, 9, 65, 18, 4, 3, "", "PAIRS", (4, 3, 3, 0, 0, 0, 0, 0, 0, 16, 12, 48, 9216, 2, 2, 1, 2, 2, 0, 0, 0, 0, 0, 78643, 32768, 0, 4, 0, 3, 5, 4, 1, 0xffff)),
    ("pairs4_33_xcd", 400, 33, 200, 301, 4, 3, "", "PAIRS", (4, 3, 3, 0, 0, 0, 0, 0, 0, 16, 6, 72, 6912, 80, 1, 1, 4, 19, 10, 0, 0, 0, 0, 131072, 7185, 0, 4, 0, 3, 5, 4, 1, 0xffff)),
    ("pairs4_33_pre", 228, 11, 65, 9, 4, 2, "", "PAIRS", (4, 3, 3, 1, 0, 0, 0, 0, 0, 4, 8, 120, 15360, 2, 3, 1, 2, 3, 0, 0, 0, 0, 0, 229880, 80099, 0, 5, 0, 3, 5, 3, 1, 0xffff)),
    ("pairs4_33_pre_xcd", 228, 180, 65, 150, 4, 2, "", "PAIRS", (4, 3, 3, 1, 0, 0, 0, 0, 0, 4, 8, 120, 15360, 80, 1, 1, 2, 38, 10, 0, 0, 0, 0, 229880, 78643, 0, 5, 0, 3, 5, 3, 1, 0xffff)),
    ("pairs4_34", 66, 8, 65, 19, 4, 3, "", "PAIRS", (4, 3, 4, 0, 0, 0, 0, 0, 0, 16, 12, 40, 7680, 2, 2, 1, 2, 2, 0, 0, 0, 0, 0, 66544, 27594, 0, 5, 0, 4, 5, 4, 1, 0xffff)),
    ("pairs4_34_xcd", 78, 602, 65, 301, 4, 3, "", "PAIRS", (4, 3, 4, 0, 0, 0, 0, 0, 0, 8, 19, 48, 14592, 80, 1, 1, 2, 38, 10, 0, 0, 0, 0, 78643, 131072, 0, 4, 0, 4, 5, 5, 1, 0xffff)),
    ("pairs4_34_pre", 175, 18, 70, 9, 4, 3, "", "PAIRS", (4, 3, 4, 1, 0, 0, 0, 0, 0, 4, 11, 88, 15488, 2, 3, 1, 2, 3, 0, 0, 0, 0, 0, 163840, 131072, 0, 5, 0, 4, 6, 5, 1, 0xffff)),
    ("pairs4_34_pre_xcd", 195, 225, 65, 150, 4, 3, "", "PAIRS", (4, 3, 4, 1, 0, 0, 0, 0, 0, 4, 10, 104, 16640, 80, 1, 1, 2, 38, 10, 0, 0, 0, 0, 196608, 98304, 0, 5, 0, 4, 6, 5, 1, 0xffff)),
    ("pairs4_35", 8, 22, 70, 18, 4, 3, "", "PAIRS", (4, 3, 5, 0, 0, 0, 0, 0, 0, 16, 25, 12, 4800, 2, 2, 1, 2, 2, 0, 0, 0, 0, 0, 7489, 80099, 0, 4, 0, 5, 4, 5, 1, 0xffff)),
    ("pairs4_35_xcd", 130, 304, 65, 301, 4, 3, "", "PAIRS", (4, 3, 5, 0, 0, 0, 0, 0, 0, 8, 14, 72, 16128, 80, 1, 1, 2, 38, 10, 0, 0, 0, 0, 131072, 66189, 0, 5, 0, 5, 5, 5, 1, 0xffff)),
    ("pairs4_35_pre", 175, 27, 70, 9, 4, 3, "", "PAIRS", (4, 3, 5, 1, 0, 0, 0, 0, 0, 4, 15, 88, 21120, 2, 3, 1, 2, 3, 0, 0, 0, 0, 0, 163840, 196608, 0, 5, 0, 5, 6, 6, 1, 0xffff)),
    ("pairs4_35_pre_xcd", 130, 375, 65, 150, 4, 3, "", "PAIRS", (4, 3, 5, 1, 0, 0, 0, 0, 0, 4, 14, 72, 16128, 80, 1, 1, 2, 38, 10, 0, 0, 0, 0, 131072, 163840, 0, 4, 0, 5, 5, 6, 1, 0xffff)),
    ("pairs4_40", 162, 8, 65, 9, 4, 3, "", "PAIRS", (4, 4, 0, 0, 0, 0, 0, 0, 0, 8, 12, 88, 16896, 2, 2, 1, 2, 2, 0, 0, 0, 0, 0, 163335, 58254, 0, 6, 0, 4, 6, 4, 1, 0xffff)),
    ("pairs4_40_xcd", 260, 128, 65, 75, 4, 3, "", "PAIRS", (4, 4, 0, 0, 0, 0, 0, 0, 0, 2, 8, 136, 17408, 80, 1, 1, 2, 38, 10, 0, 0, 0, 0, 262144, 111848, 0, 6, 0, 5, 7, 5, 1, 0xffff)),
    ("pairs4_46_pre", 136, 19, 65, 9, 4, 3, "", "PAIRS", (4, 4, 6, 1, 0, 0, 0, 0, 0, 4, 14, 76, 17024, 2, 3, 1, 2, 3, 0, 0, 0, 0, 0, 137121, 138353, 0, 6, 0, 6, 6, 6, 1, 0xffff)),
    ("pairs4_46_pre_xcd", 228, 158, 65, 75, 4, 3, "", "PAIRS", (4, 4, 6, 1, 0, 0, 0, 0, 0, 2, 10, 120, 19200, 80, 1, 1, 2, 38, 10, 0, 0, 0, 0, 229880, 138062, 0, 7, 0, 6, 7, 6, 1, 0xffff)),
    ("up_11", 26, 9, 65, 9, 4, 2, "", "UP", (0, 1, 1, 0, 0, 0, 0, 0, 0, 6, 0, 0, 0, 1, 2, 1, 0, 0, 0, 0, 0, 0, 6, 26214, 65536, 0, 2, 0, 1, 2, 2, 0, 0xffff)),
    ("up_12", 26, 8, 65, 9, 4, 2, "", "UP", (0, 1, 2, 0, 0, 0, 0, 0, 0, 6, 0, 0, 0, 1, 2, 1, 0, 0, 0, 0, 0, 0, 6, 26214, 58254, 0, 2, 0, 2, 2, 2, 0, 0xffff)),
    ("up_23", 8, 9, 70, 9, 4, 3, "", "UP", (0, 2, 3, 0, 0, 0, 0, 0, 0, 6, 0, 0, 0, 1, 2, 1, 0, 0, 0, 0, 0, 0, 6, 7489, 65536, 0, 3, 0, 3, 4, 4, 0, 0xffff)),
    ("up_24", 8, 8, 70, 9, 4, 3, "", "UP", (0, 2, 4, 0, 0, 0, 0, 0, 0, 6, 0, 0, 0, 1, 2, 1, 0, 0, 0, 0, 0, 0, 6, 7489, 58254, 0, 4, 0, 4, 4, 4, 0, 0xffff)),
    ("window3", 16, 8, 65, 19, 3, 2, "", "WINDOW", (3, 0, 0, 0, 0, 0, 0, 0, 0, 16, 9, 18, 648, 2, 2, 1, 0, 0, 0, 0, 0, 0, 0, 16131, 27594, 0, 2, 0, 2, 2, 2, 0, 0x8000)),
    ("window3_uniform", 520, 11, 65, 9, 3, 3, "", "WINDOW", (3, 0, 0, 0, 0, 0, 0, 0, 1, 8, 14, 515, 28840, 2, 2, 1, 0, 0, 0, 0, 0, 0, 0, 524288, 80099, 0, 11, 0, 5, 11, 5, 0, 0xffff)),
    ("window4", 16, 8, 65, 19, 4, 2, "", "WINDOW", (4, 0, 0, 0, 0, 0, 0, 0, 0, 16, 9, 18, 648, 2, 2, 1, 0, 0, 0, 0, 0, 0, 0, 16131, 27594, 0, 2, 0, 2, 2, 2, 0, 0xffff)),
    ("window4_uniform", 520, 11, 65, 9, 4, 3, "", "WINDOW", (4, 0, 0, 0, 0, 0, 0, 0, 1, 8, 14, 515, 28840, 2, 2, 1, 0, 0, 0, 0, 0, 0, 0, 524288, 80099, 0, 11, 0, 5, 11, 5, 0, 0xffff)),
    ("direct3_small", 252, 32, 9, 9, 3, 3, "", "DIRECT", (3, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1795, 0, 1, 3, 1, 0, 0, 0, 0, 0, 0, 0, 1835008, 233016, 0, 31, 0, 7, 31, 7, 0, 0xffff)),
    ("direct4_small", 252, 32, 9, 9, 4, 3, "", "DIRECT", (4, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1795, 0, 1, 3, 1, 0, 0, 0, 0, 0, 0, 0, 1835008, 233016, 0, 31, 0, 7, 31, 7, 0, 0xffff)),
    ("gather_1_small", 9, 18, 9, 9, 4, 2, "", "GATHER", (0, 1, 0, 0, 0, 0, 0, 0, 0, 4, 0, 0, 0, 1, 3, 1, 0, 0, 0, 0, 0, 0, 0, 65536, 131072, 0, 1, 0, 2, 2, 3, 0, 0xffff)),
    ("nearest3_small", 14, 8, 9, 19, 3, 0, "", "NEAREST", (3, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 5, 1, 0, 0, 0, 0, 0, 0, 0, 101944, 27594, 0, 0, 0, 0, 0, 0, 0, 0x0)),
    ("nearest4_small", 14, 8, 9, 19, 4, 0, "", "NEAREST", (4, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 5, 1, 0, 0, 0, 0, 0, 0, 0, 101944, 27594, 0, 0, 0, 0, 0, 0, 0, 0x0)),
    ("pairs3_22_small", 8, 9, 9, 18, 3, 2, "", "PAIRS", (3, 2, 2, 0, 0, 0, 0, 0, 0, 16, 11, 36, 6336, 1, 2, 1, 1, 2, 0, 0, 0, 0, 0, 58254, 32768, 0, 2, 0, 2, 2, 2, 1, 0x8000)),
    ("pairs4_30_small", 9, 19, 9, 9, 4, 3, "", "PAIRS", (4, 3, 0, 0, 0, 0, 0, 0, 0, 8, 22, 40, 14080, 1, 2, 1, 1, 2, 0, 0, 0, 0, 0, 65536, 138353, 0, 4, 0, 6, 4, 6, 1, 0xffff)),
    ("up_24_small", 8, 8, 9, 9, 4, 3, "", "UP", (0, 2, 4, 0, 0, 0, 0, 0, 0, 6, 0, 0, 0, 1, 2, 1, 0, 0, 0, 0, 0, 0, 6, 58254, 58254, 0, 4, 0, 4, 4, 4, 0, 0xffff)),
    ("window3_small", 8, 8, 9, 19, 3, 2, "", "WINDOW", (3, 0, 0, 0, 0, 0, 0, 0, 0, 16, 9, 58, 2088, 1, 2, 1, 0, 0, 0, 0, 0, 0, 0, 58254, 27594, 0, 2, 0, 2, 2, 2, 0, 0x8000)),
    ("window4_small", 8, 8, 9, 19, 4, 2, "", "WINDOW", (4, 0, 0, 0, 0, 0, 0, 0, 0, 16, 9, 58, 2088, 1, 2, 1, 0, 0, 0, 0, 0, 0, 0, 58254, 27594, 0, 2, 0, 2, 2, 2, 0, 0xffff)),
    ("pairs3_narrow", 1, 72, 9, 9, 3, 2, "", "PAIRS", (3, 2, 0, 0, 0, 0, 0, 0, 0, 8, 65, 12, 12480, 1, 2, 1, 1, 2, 0, 0, 0, 0, 0, 7281, 524288, 0, 2, 0, 8, 2, 9, 1, 0xffff)),
    ("pairs4_narrow", 1, 72, 9, 9, 4, 2, "", "PAIRS", (4, 2, 0, 0, 0, 0, 0, 0, 0, 8, 65, 12, 12480, 1, 2, 1, 1, 2, 0, 0, 0, 0, 0, 7281, 524288, 0, 2, 0, 8, 2, 9, 1, 0xffff)),
    ("up_narrow", 1, 1, 9, 9, 4, 2, "", "UP", (0, 1, 2, 0, 0, 0, 0, 0, 0, 6, 0, 0, 0, 1, 2, 1, 0, 0, 0, 0, 0, 0, 6, 7281, 7281, 0, 2, 0, 2, 2, 2, 0, 0xffff)),
    ("window3_narrow", 1, 2, 9, 18, 3, 2, "PB_NO_PAIRS=1", "WINDOW", (3, 0, 0, 0, 0, 0, 0, 0, 0, 16, 4, 9, 144, 1, 2, 1, 0, 0, 0, 0, 0, 0, 0, 7281, 7281, 0, 2, 0, 2, 2, 2, 0, 0x8000)),
    ("window4_narrow", 1, 2, 9, 18, 4, 2, "PB_NO_PAIRS=1", "WINDOW", (4, 0, 0, 0, 0, 0, 0, 0, 0, 16, 4, 9, 144, 1, 2, 1, 0, 0, 0, 0, 0, 0, 0, 7281, 7281, 0, 2, 0, 2, 2, 2, 0, 0xffff)),
    ("copy", 70, 19, 70, 19, 4, 3, "", "COPY", (0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0x0)),
    ("refused", 130, 130, 2, 3, 4, 3, "", "REFUSED", (0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0, 4259840, 2839893, 0, 0, 0, 0, 68, 47, 0, 0x0)),
    ("not_fused_window", 16, 8, 65, 19, 4, 2, "", "NOT_FUSED", (0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 2, 5, 1, 0, 0, 0, 0, 0, 0, 0, 16131, 27594, 0, 2, 0, 2, 2, 2, 0, 0xffff)),
    ("double_small", 20, 10, 40, 20, 4, 2, "", "DOUBLE", (0, 0, 0, 0, 0, 0, 0, 0, 0, 3, 0, 0, 0, 8, 1, 1, 0, 0, 0, 1, 1, 4, 0, 32768, 32768, 0, 2, 0, 2, 2, 2, 0, 0xffff)),
    ("half_bilinear_small", 40, 20, 20, 10, 4, 2, "", "HALF", (0, 0, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 131072, 131072, 0, 2, 0, 2, 3, 3, 0, 0xffff)),
    ("half3_hyper_small", 40, 20, 20, 10, 3, 3, "", "HALF3", (0, 0, 0, 0, 0, 0, 1, 0, 0, 6, 0, 0, 0, 8, 1, 1, 0, 0, 0, 1, 1, 2, 0, 131072, 131072, 0, 4, 0, 4, 5, 5, 0, 0xffff)),
    ("half_bilinear_strips", 140, 38, 70, 19, 4, 2, "PBH_ALIGNED=0", "HALF", (0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 131072, 131072, 0, 2, 0, 2, 3, 3, 0, 0xffff)),
    ("half_hyper_strips", 140, 38, 70, 19, 4, 3, "PBH_ALIGNED=0", "HALF", (0, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 131072, 131072, 0, 4, 0, 4, 5, 5, 0, 0xffff)),
    ("direct3_narrow", 30, 27, 1, 1, 3, 3, "", "DIRECT", (3, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1923, 0, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0, 1966080, 1769472, 0, 32, 0, 29, 33, 30, 0, 0xffff)),
    ("direct4_narrow", 30, 27, 1, 1, 4, 3, "", "DIRECT", (4, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1923, 0, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0, 1966080, 1769472, 0, 32, 0, 29, 33, 30, 0, 0xffff)),
    ("gather_narrow", 3, 3, 1, 1, 4, 3, "", "GATHER", (0, 3, 0, 0, 0, 0, 0, 0, 0, 4, 0, 0, 0, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0, 196608, 196608, 0, 6, 0, 6, 6, 6, 0, 0xffff)),
]]
BY_NAME = {r.name: r for r in ROWS}
assert len(BY_NAME) == len(ROWS)

# every key the dispatcher can return, written out: 88.  PAIRS: (channels, NP, NY, PRE, tile order); NY > 0 only for the six short filters <2, 2>, <2, 3>, <3, 3>,
# <3, 4>, <3, 5>, <4, 6>, each again as PRE for tiles of at most four rows.  Not among them (NOT_REACHED): <4, 6> without PRE, and <2, 2> with PRE on 4-byte pixels
REACHABLE = {
    ("COPY",), ("REFUSED",), ("NOT_FUSED",),
    ("NEAREST", 3), ("NEAREST", 4),
    ("DOUBLE",),
    ("HALF3", 0), ("HALF3", 1),
    ("HALF", 0, 0), ("HALF", 0, 1), ("HALF", 1, 0), ("HALF", 1, 1),
    ("UP", 1, 1), ("UP", 1, 2), ("UP", 2, 3), ("UP", 2, 4),
    ("GATHER", 1), ("GATHER", 2), ("GATHER", 3), ("GATHER", 4),
    ("PAIRS", 3, 0, 0, 0, "grid"), ("PAIRS", 3, 0, 0, 0, "xcd"), ("PAIRS", 3, 1, 0, 0, "grid"), ("PAIRS", 3, 1, 0, 0, "xcd"),
    ("PAIRS", 3, 2, 0, 0, "grid"), ("PAIRS", 3, 2, 0, 0, "xcd"), ("PAIRS", 3, 3, 0, 0, "grid"), ("PAIRS", 3, 3, 0, 0, "xcd"),
    ("PAIRS", 3, 4, 0, 0, "grid"), ("PAIRS", 3, 4, 0, 0, "xcd"),
    ("PAIRS", 3, 2, 2, 0, "grid"), ("PAIRS", 3, 2, 2, 0, "xcd"), ("PAIRS", 3, 2, 2, 1, "grid"), ("PAIRS", 3, 2, 2, 1, "xcd"),
    ("PAIRS", 3, 2, 3, 0, "grid"), ("PAIRS", 3, 2, 3, 0, "xcd"), ("PAIRS", 3, 2, 3, 1, "grid"), ("PAIRS", 3, 2, 3, 1, "xcd"),
    ("PAIRS", 3, 3, 3, 0, "grid"), ("PAIRS", 3, 3, 3, 0, "xcd"), ("PAIRS", 3, 3, 3, 1, "grid"), ("PAIRS", 3, 3, 3, 1, "xcd"),
    ("PAIRS", 3, 3, 4, 0, "grid"), ("PAIRS", 3, 3, 4, 0, "xcd"), ("PAIRS", 3, 3, 4, 1, "grid"), ("PAIRS", 3, 3, 4, 1, "xcd"),
    ("PAIRS", 3, 3, 5, 0, "grid"), ("PAIRS", 3, 3, 5, 0, "xcd"), ("PAIRS", 3, 3, 5, 1, "grid"), ("PAIRS", 3, 3, 5, 1, "xcd"),
    ("PAIRS", 3, 4, 6, 1, "grid"), ("PAIRS", 3, 4, 6, 1, "xcd"),
    ("PAIRS", 4, 0, 0, 0, "grid"), ("PAIRS", 4, 0, 0, 0, "xcd"), ("PAIRS", 4, 1, 0, 0, "grid"), ("PAIRS", 4, 1, 0, 0, "xcd"),
    ("PAIRS", 4, 2, 0, 0, "grid"), ("PAIRS", 4, 2, 0, 0, "xcd"), ("PAIRS", 4, 3, 0, 0, "grid"), ("PAIRS", 4, 3, 0, 0, "xcd"),
    ("PAIRS", 4, 4, 0, 0, "grid"), ("PAIRS", 4, 4, 0, 0, "xcd"),
    ("PAIRS", 4, 2, 2, 0, "grid"), ("PAIRS", 4, 2, 2, 0, "xcd"),
    ("PAIRS", 4, 2, 3, 0, "grid"), ("PAIRS", 4, 2, 3, 0, "xcd"), ("PAIRS", 4, 2, 3, 1, "grid"), ("PAIRS", 4, 2, 3, 1, "xcd"),
    ("PAIRS", 4, 3, 3, 0, "grid"), ("PAIRS", 4, 3, 3, 0, "xcd"), ("PAIRS", 4, 3, 3, 1, "grid"), ("PAIRS", 4, 3, 3, 1, "xcd"),
    ("PAIRS", 4, 3, 4, 0, "grid"), ("PAIRS", 4, 3, 4, 0, "xcd"), ("PAIRS", 4, 3, 4, 1, "grid"), ("PAIRS", 4, 3, 4, 1, "xcd"),
    ("PAIRS", 4, 3, 5, 0, "grid"), ("PAIRS", 4, 3, 5, 0, "xcd"), ("PAIRS", 4, 3, 5, 1, "grid"), ("PAIRS", 4, 3, 5, 1, "xcd"),
    ("PAIRS", 4, 4, 6, 1, "grid"), ("PAIRS", 4, 4, 6, 1, "xcd"),
    ("WINDOW", 3, 0), ("WINDOW", 3, 1), ("WINDOW", 4, 0), ("WINDOW", 4, 1),
    ("DIRECT", 3), ("DIRECT", 4),
}
# keys per family, counted by hand from the dispatcher: a slip in the list above shows here
REACHABLE_COUNTS = {"COPY": 1, "REFUSED": 1, "NOT_FUSED": 1, "NEAREST": 2, "DOUBLE": 1, "HALF3": 2, "HALF": 4, "UP": 4, "GATHER": 4, "PAIRS": 62, "WINDOW": 4, "DIRECT": 2}
# what pb_dimension's tap counts prove unreachable, and was deleted from the dispatcher for it (four instantiations each: OPQ x PbEpi)
UP_ARGUMENT = ("one filter serves both axes; enlarging or keeping a side, BILINEAR has 2 taps (one pair, 1-2 tap rows) and HYPER 4 of which at least 3 are non-zero "
               "over the phases a frame takes (pixel 0's phase 0 weights taps 0 and 1, the last pixel's phase tap 2; a kept side is [1 6 1] / 8): two pairs, 3-4 tap rows")
UNREACHABLE = [("k_pb_up<1, 3>", UP_ARGUMENT), ("k_pb_up<1, 4>", UP_ARGUMENT), ("k_pb_up<2, 1>", UP_ARGUMENT), ("k_pb_up<2, 2>", UP_ARGUMENT)]
# arms the sweep never returns and no argument from the tap counts alone excludes: kept in the dispatcher, with the bound they were looked for up to
SWEEP_BOUND = "destinations up to 200 x 301, ratios from 1:9 to 40:1 per axis (test_no_geometry_leaves_the_listed_keys); a search of sides up to 1100 found none either"
NOT_REACHED = [
    ("k_pb_pairs<3 | 4, 4, 6, 0> (both tile orders)", "tiles of 8 rows need 6 tap rows and 6-7 taps in at most 24 KB: the smallest such window (steps just over 2, HYPER) "
     "is 72 pairs x 22 rows x 16 bytes = 25344", SWEEP_BOUND),
    ("k_pb_pairs<4, 2, 2, 1> (both tile orders)", "4-byte pixels with a 2 x 2-pair box and tiles of at most 4 rows were only seen at integer steps, which k_pb_gather takes",
     SWEEP_BOUND),
]


def pitches(r):
    return align(r.sw * r.ch, 16), align(r.dw * r.ch, 16) + 16


def set_tune(tune, r):
    """the row's switch on, the others the rows use at their defaults"""
    want = dict([r.tune.split("=")]) if r.tune else {}
    for name in ("PB_NO_PAIRS", "PBH_ALIGNED", "PB_UP_RB", "PB_CHAIN_GROUP"):
        tune(name, int(want.get(name, -1)))


def row_mode(r):
    return lib.PB_PLAN_CHAIN if r.path == "NOT_FUSED" else lib.PB_PLAN_SCALE


def plan(r, ops, src_bits=0, dst_bits=0, nframes=1, mode=None, flags=0):
    irow, orow = pitches(r)
    return ops.pixbuf_plan(r.sw, r.sh, r.dw, r.dh, r.ch, r.interp | flags, irow=irow, orow=orow, src_bits=src_bits, dst_bits=dst_bits, nframes=nframes,
                           mode=row_mode(r) if mode is None else mode)


def key(d):
    """the family and its template arguments (k_pb_pairs: and the tile order): what REACHABLE lists"""
    p = d["path"]
    if p in ("NEAREST", "DIRECT"):
        return (p, d["ch"])
    if p == "HALF3":
        return (p, d["hyper"])
    if p == "HALF":
        return (p, d["hyper"], d["aligned"])
    if p == "UP":
        return (p, d["np"], d["ny"])
    if p == "GATHER":
        return (p, d["np"])
    if p == "PAIRS":
        return (p, d["ch"], d["np"], d["ny"], d["pre"], "xcd" if d["per_xcd"] else "grid")
    if p == "WINDOW":
        return (p, d["ch"], d["uniform"])
    return (p,)


def row_dict(r):
    return dict(zip(PLAN_FIELDS, r.plan), path=r.path)


def family(r):
    return (r.path, r.ch) if r.path in ("NEAREST", "PAIRS", "WINDOW", "DIRECT") else (r.path,)


def describe(r, d):
    return "%s: %dx%d -> %dx%d, %d channels, interp %d, %s: planned %s" % (r.name, r.sw, r.sh, r.dw, r.dh, r.ch, r.interp, r.tune or "no switch", key(d))


def same_plan(d, r, **changed):
    want = dict(row_dict(r), **changed)
    bad = {f: (d[f], want[f]) for f in PLAN_FIELDS + ("path",) if d[f] != want[f]}
    assert not bad, "%s: (query, table) differ in %s" % (describe(r, d), bad)


def rows_source():
    """ROWS again with the plans the query gives now (python -c 'from tests import test_pixbuf_plans as t; print(t.rows_source())'): for a new row, write it
    with an empty plan and take its line from here"""
    from lives_amd import ops as o
    lib.load()
    out = []
    for r in ROWS:
        for name in ("PB_NO_PAIRS", "PBH_ALIGNED"):
            o.tuning(name, int(dict([r.tune.split("=")]).get(name, -1)) if r.tune else -1)
        d = plan(r, o)
        out.append('    ("%s", %d, %d, %d, %d, %d, %d, "%s", "%s", (%s)),' % (r.name, r.sw, r.sh, r.dw, r.dh, r.ch, r.interp, r.tune, d["path"],
                                                                          ", ".join("0x%x" % d[f] if f == "rnd" else str(d[f]) for f in PLAN_FIELDS)))
    for name in ("PB_NO_PAIRS", "PBH_ALIGNED"):
        o.tuning(name, -1)
    return "\n".join(out)


@pytest.fixture
def ops_cpu():
    """lives_amd.ops without a device: only its host-side calls (the plan query, the weight tables, the tuning table) are used"""
    from lives_amd import ops
    lib.load()
    return ops


# ------------------------------------------------------------------------------------------------------------------ CPU: the table against the dispatcher
def test_every_row_takes_the_plan_written_in_the_table(ops_cpu, tune):
    for r in ROWS:
        set_tune(tune, r)
        d = plan(r, ops_cpu)
        same_plan(d, r)
        assert d["rc"] == (-3 if r.path == "REFUSED" else 0), describe(r, d)


def test_the_table_covers_exactly_what_the_dispatcher_can_return(ops_cpu, tune):
    got = set()
    for r in ROWS:
        set_tune(tune, r)
        got.add(key(plan(r, ops_cpu)))
    assert got == REACHABLE, "rows without a listed key: %s; listed keys without a row: %s" % (sorted(got - REACHABLE, key=str), sorted(REACHABLE - got, key=str))
    assert {f: sum(1 for k in REACHABLE if k[0] == f) for f in REACHABLE_COUNTS} == REACHABLE_COUNTS and len(REACHABLE) == 88


SWEEP_RATIOS = [1 / 9, 1 / 4, 1 / 3, 0.4, 0.5, 1 / 1.5, 1 / 1.2, 1, 1.01, 1.2, 1.5, 1.7, 1.9, 2, 2.1, 2.5, 3, 3.5, 4, 4.5, 5, 5.5, 6, 7, 8, 10, 12, 16, 20, 28, 40]


def test_no_geometry_leaves_the_listed_keys(ops_cpu, tune):
    """a sweep of the query: destinations 9 / 65 / 70 / 200 wide and 9 / 18 / 19 / 75 / 150 / 301 high (both sides of the 64 tiles at which k_pb_pairs changes its
    tile order), sources at 31 ratios per axis from 1:9 (enlarging) over 1 (a side kept) to 40:1 (past the refusal), whole and fractional, both filters, both
    channel counts, with and without PB_NO_PAIRS; NEAREST, the chain's call and k_pb_half's PBH_ALIGNED = 0 on a few of them.  The keys returned are exactly
    REACHABLE: an arm that goes dead, or a new one, fails here"""
    seen = set()

    def ask(sw, sh, dw, dh, ch, interp, **kw):
        d = ops_cpu.pixbuf_plan(sw, sh, dw, dh, ch, interp, irow=align(sw * ch, 16), orow=align(dw * ch, 16) + 16, **kw)
        k = key(d)
        assert k in REACHABLE, "%dx%d -> %dx%d, %d channels, interp %d, %s: %s" % (sw, sh, dw, dh, ch, interp, kw, k)
        seen.add(k)
        return d

    for nop in (0, 1):
        tune("PB_NO_PAIRS", 1 if nop else -1)
        for dw in (9, 65, 70, 200):
            for dh in (9, 18, 19, 75, 150, 301):
                for rx in SWEEP_RATIOS:
                    for ry in SWEEP_RATIOS:
                        sw, sh = max(1, round(dw * rx)), max(1, round(dh * ry))
                        if sw * sh > 400000:
                            continue
                        for ch in (3, 4):
                            for interp in (2, 3):
                                d = ask(sw, sh, dw, dh, ch, interp)
                                if ch == 4 and (sw, sh) != (dw, dh) and rx in (0.4, 1, 2, 2.5, 4.5, 12) and dh in (19, 150):
                                    e = ask(sw, sh, dw, dh, 4, interp, nframes=3, mode=lib.PB_PLAN_CHAIN)
                                    if d["path"] in ("UP", "GATHER", "PAIRS"):
                                        assert e["path"] == d["path"] and e["epi"] == 1, (sw, sh, dw, dh, interp)
                                    elif d["path"] in ("DOUBLE", "HALF"):           # scale-only kernels: the chain's call falls through to the general ones
                                        assert e["path"] in ("UP", "GATHER", "PAIRS", "NOT_FUSED"), (sw, sh, dw, dh, interp)
                                    else:
                                        assert e["path"] == "NOT_FUSED", (sw, sh, dw, dh, interp)
                            if (rx, ry) in ((1.5, 0.4), (0.4, 1.5), (1, 1)):
                                ask(sw, sh, dw, dh, ch, 0)
    tune("PB_NO_PAIRS", -1)
    tune("PBH_ALIGNED", 0)
    for interp in (2, 3):
        assert ask(140, 38, 70, 19, 4, interp)["aligned"] == 0
    assert seen == REACHABLE, "never returned: %s" % sorted(REACHABLE - seen, key=str)


def test_query_refuses_what_the_entry_points_refuse(ops_cpu):
    for kw in (dict(channels=2), dict(interp=1), dict(irow=8), dict(orow=8), dict(nframes=0), dict(nframes=65), dict(mode=7), dict(src_bits=2), dict(dst_bits=1),
               dict(irow=402), dict(mode=lib.PB_PLAN_CHAIN, channels=3)):
        with pytest.raises(lib.LgpuError):
            ops_cpu.pixbuf_plan(100, 50, 67, 37, **kw)
    for g in ((0, 5, 4, 4), (4, 4, 4, 0), (32768, 4, 100, 4), (4, 4, 4, 32768)):
        with pytest.raises(lib.LgpuError):
            ops_cpu.pixbuf_plan(*g)
    with pytest.raises(lib.LgpuError):
        ops_cpu.pixbuf_plan(64, 64, 64, 64, mode=lib.PB_PLAN_CHAIN)
    # 3-byte pixels have no alignment demand
    assert ops_cpu.pixbuf_plan(100, 50, 67, 37, channels=3, irow=301, orow=203, src_bits=1, dst_bits=3)["path"] == "PAIRS"
    # the flag is ignored where no lighter form exists, and reported where one does
    assert ops_cpu.pixbuf_plan(100, 50, 67, 37, interp=3 | OPAQUE)["opq"] == 1 and ops_cpu.pixbuf_plan(100, 50, 67, 37, channels=3, interp=3 | OPAQUE)["opq"] == 0
    d = ops_cpu.pixbuf_plan(120, 120, 2, 2)
    assert (d["path"], d["rc"], d["n_x"], d["n_y"]) == ("REFUSED", -3, 63, 63)


def test_the_tuning_switches_are_read_as_the_launch_reads_them(ops_cpu, tune):
    r = BY_NAME["up_24"]
    assert plan(r, ops_cpu)["rb"] == 6 and ops_cpu.pixbuf_plan(2000, 1500, 2400, 2500)["rb"] == 8
    tune("PB_UP_RB", 5)
    d = plan(r, ops_cpu)
    assert (d["rb"], d["tile_h"], d["gy"]) == (5, 5, -(-r.dh // 5))
    tune("PB_UP_RB", -1)
    tune("PB_NO_PAIRS", 1)
    assert plan(r, ops_cpu)["path"] == "WINDOW"


NO_KERNEL = ("COPY", "REFUSED", "NOT_FUSED")


def taps_reach(r, d, L):
    """(left, right, top, bottom): the used taps of the first / the last destination pixel lie outside the frame, so that the clamp works at that border"""
    import ctypes
    v = [ctypes.c_int() for _ in range(4)]
    assert L.lgpu_pixbuf_weights(r.interp, r.sw, r.sh, r.dw, r.dh, *[ctypes.byref(x) for x in v], None, 0) == 0
    xoff, yoff = v[2].value, v[3].value
    return ((xoff >> 16) + d["tx0"] < 0, (((r.dw - 1) * d["x_step"] + xoff) >> 16) + d["tx1"] - 1 >= r.sw,
            (yoff >> 16) + d["ty0"] < 0, (((r.dh - 1) * d["y_step"] + yoff) >> 16) + d["ty1"] - 1 >= r.sh)


def band_rows(d):
    """destination rows per tile, band or grid row (k_pb_double: 3 source rows; k_pb_half's bands depend on the device)"""
    return {"PAIRS": d["tile_h"], "WINDOW": d["tile_h"], "UP": d["tile_h"], "GATHER": 4, "HALF3": 6, "NEAREST": 4, "DIRECT": 4, "DOUBLE": 6}.get(d["path"], 0)


def test_rows_keep_to_the_shape_rules(ops_cpu):
    """Rows other than *_small / *_narrow: at least two tile columns with a partial last one (dw > 64, no multiple of 64); at least two tile rows or bands with a
    partial last one; per-XCD rows at least 64 tiles and no multiple of 8, so that the last XCD's run is padded.  The used taps reach past the frame wherever the
    filter can: HYPER at all four borders; BILINEAR at both ends of an axis it enlarges (its box of source pixels [j step, (j + 1) step) never leaves the frame
    when it reduces, and a kept axis is one tap).  Every family has a row clamped at all four borders, a row with dw < 64 and -- where a frame can be
    narrower than its tap row -- such a row.  Nothing is larger than a few hundred pixels a side but the sources of k_pb_direct and of the 16:1 .. 20:1 rows"""
    L = lib.load()
    four, small, narrow = set(), set(), set()
    for r in ROWS:
        d = row_dict(r)
        assert r.dw <= 400 and r.dh <= 400 and r.sw * r.sh <= 100000, r.name
        if r.path in NO_KERNEL:
            continue
        fam = family(r)
        if r.name.endswith("_small") or r.name.endswith("_narrow"):
            assert r.dw < 64, r.name
            small.add(fam)
            if r.name.endswith("_narrow"):
                assert r.sw < d["tx1"] - d["tx0"], r.name
                narrow.add(fam)
            continue
        assert r.dw > 64 and r.dw % 64, r.name
        bh = band_rows(d)
        assert bh == 0 or (r.dh > bh and r.dh % bh), "%s: %d rows in bands of %d" % (r.name, r.dh, bh)
        if d["per_xcd"]:
            tiles = d["tiles_x"] * d["tiles_y"]
            assert tiles >= 64 and tiles % 8 and d["gx"] == 8 * d["per_xcd"] > tiles, r.name
        elif r.path == "PAIRS":
            assert d["tiles_x"] >= 2 and d["tiles_y"] >= 2 and d["tiles_x"] * d["tiles_y"] < 64, r.name
        if r.interp == 0:
            four.add(fam)
            continue
        left, right, top, bottom = taps_reach(r, d, L)
        if r.interp == 3:
            assert left and right and top and bottom, "%s: %s" % (r.name, (left, right, top, bottom))
        else:
            assert left == right == (r.dw > r.sw) or (right and r.dw <= r.sw), "%s: %s" % (r.name, (left, right))
            assert top == bottom == (r.dh > r.sh) or (bottom and r.dh <= r.sh), "%s: %s" % (r.name, (top, bottom))
        if left and right and top and bottom:
            four.add(fam)
    fams = {family(r) for r in ROWS if r.path not in NO_KERNEL}
    assert four == fams, "no row clamped at all four borders: %s" % sorted(fams - four, key=str)
    assert small == fams, "no row with dw < 64: %s" % sorted(fams - small, key=str)
    # NEAREST has no taps; the exact 2:1 / 1:2 kernels ask for sources at least as wide as their 4 resp. 2 taps
    assert narrow == {f for f in fams if f[0] in ("UP", "GATHER", "PAIRS", "WINDOW", "DIRECT")}, sorted(narrow, key=str)


# ------------------------------------------------------------------------------------------------------------------ the table in docs/KERNELS.md
DOC_KEYS = [
    (("COPY",), "`lgpu_copy_rows`", "same size (as the library does)"),
    (("REFUSED",), "none", "more than 1000 taps (`n_x * n_y`): the library's two-step scaler; `LGPU_E_UNSUPPORTED`, nothing written"),
    (("NOT_FUSED",), "none", "the chain's call where none of `k_pb_up`, `k_pb_gather`, `k_pb_pairs` has the ratio (or NEAREST): the chain runs its stages one after the other"),
    (("NEAREST",), "`k_pb_nearest<ch>`", "interp 0"),
    (("DOUBLE",), "`k_pb_double<0>`", "4-byte pixels, exact 1:2 on both axes, `sw` even, source 8-byte and destination 16-byte aligned (frames and pitches), the (1, 3) / (3, 1) table"),
    (("HALF3",), "`k_pb_half3<hyper>`", "3-byte pixels, exact 2:1 on both axes, `sw % 8 == 0`, 4-byte aligned frames and pitches"),
    (("HALF",), "`k_pb_half<0, hyper, 0, aligned>`", "4-byte pixels, exact 2:1 on both axes, `sw % 4 == 0`, source 16-byte and destination 8-byte aligned; `aligned` 0 only under `PBH_ALIGNED=0`"),
    (("UP",), "`k_pb_up<np, ny, opq, epi>`", "4-byte pixels, no side reduced, every weight below 65536; `np = ceil(taps / 2)`, `ny` tap rows of the used box"),
    (("GATHER",), "`k_pb_gather<np, epi, opq>`", "4-byte pixels, whole steps on both axes (one phase for the frame), every weight below 65536, at most 8 taps a row"),
    (("PAIRS",), "`k_pb_pairs<ch, np, ny, pre, opq, epi>`", "every weight of the used phases below 65536 and a window of at least one tile row within 24 KB; `np = (taps + 2) / 2` "
     "up to 4 (0: any), `ny` at compile time for the six short filters (0: any), `pre` for tiles of at most 4 rows; xcd: at least 64 tiles"),
    (("WINDOW",), "`k_pb_window<ch, uniform>`", "a 65536 weight among the used phases (most BILINEAR enlargements), or `PB_NO_PAIRS`, and a window within 48 KB; `uniform`: a whole x step"),
    (("DIRECT",), "`k_pb_direct<ch>`", "no window fits: neither `k_pb_pairs`' 24 KB nor `k_pb_window`'s 48 KB at one-row tiles"),
]


def key_label(k):
    if k[0] == "PAIRS":
        return "<%d, %d, %d, %d, opq, epi>, %s order" % (k[1:5] + ("per-XCD" if k[5] == "xcd" else "plain grid",))
    if k[0] == "UP":
        return "<%d, %d, opq, epi>" % k[1:]
    if k[0] == "GATHER":
        return "<%d, epi, opq>" % k[1:]
    if k[0] == "DOUBLE":
        return "<0>"
    if k[0] == "HALF":
        return "<0, %d, 0, %d>" % k[1:]
    return "<%s>" % ", ".join(str(x) for x in k[1:]) if len(k) > 1 else ""


def doc_table():
    """the key table of docs/KERNELS.md, generated from ROWS (python -c 'from tests import test_pixbuf_plans as t; print(t.doc_table())')"""
    out = ["| path (`lgpu_debug_pixbuf_plan`) | kernel | reached when |", "|---|---|---|"]
    out += ["| `%s` | %s | %s |" % (path, kernel, cond) for (path,), kernel, cond in DOC_KEYS]
    out += ["", "One line per key (`REACHABLE`), with the rows of `tests/test_pixbuf_plans.py` that reach it (sw x sh -> dw x dh, channels, interp):", "",
            "| key | kernel | rows |", "|---|---|---|"]
    for (path,), kernel, cond in DOC_KEYS:
        groups = {}
        for r in ROWS:
            if r.path == path:
                groups.setdefault(key(row_dict(r)), []).append(r)
        name = kernel.strip("`").split("<")[0]
        for k in sorted(groups, key=str):
            out.append("| `%s` | %s | %s |" % (" ".join(str(x) for x in k), "`%s%s`" % (name, key_label(k)) if name.startswith("k_") else kernel, ", ".join(
                "`%s` (%dx%d -> %dx%d, %d, %d%s)" % (r.name, r.sw, r.sh, r.dw, r.dh, r.ch, r.interp, ", " + r.tune if r.tune else "") for r in groups[k])))
    out += ["", "Deleted from the dispatcher, with the argument (`UNREACHABLE`):", ""]
    out += ["- `%s` (`opq` x `epi`: four instantiations): %s" % u for u in UNREACHABLE]
    out += ["", "Kept, and not reached up to the sweep's bound (`NOT_REACHED`):", ""]
    out += ["- `%s`: %s; bound: %s" % n for n in NOT_REACHED]
    return "\n".join(out) + "\n"


def test_the_table_in_the_docs_is_the_one_generated_from_the_rows():
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "docs", "KERNELS.md")).read()
    assert "#### Which kernel a pixbuf scale takes" in text
    assert doc_table() in text, "docs/KERNELS.md: replace the key table of the pixbuf section with doc_table()'s output"


# ------------------------------------------------------------------------------------------------------------------ sources and the oracle's frames
FILL = 0xA5
ALPHA_MIXES = ("random", "opaque", "0 / 255 / 7")
_WANT = {}


def make_src(rng, sw, sh, ch, irow, amode):
    """a source frame; 4-byte pixels with alpha random, 255 everywhere, or from {0, 255, 7} (zero-alpha pixels occur)"""
    src = rng.integers(0, 256, (sh, irow), dtype=np.uint8)
    if ch == 4 and amode == 1:
        src[:, 3:sw * 4:4] = 255
    elif ch == 4 and amode == 2:
        src[:, 3:sw * 4:4] = rng.choice(np.array([0, 255, 7], np.uint8), (sh, sw))
    return src


def oracle_scale(orc, tag, sw, sh, dw, dh, ch, interp, irow, amode, seed):
    """(source frame, the oracle's frame, its return code), computed once per case and shared by the tests of a session"""
    if tag not in _WANT:
        src = make_src(np.random.default_rng(seed), sw, sh, ch, irow, amode)
        want = np.zeros((dh, dw * ch), np.uint8)
        rc = orc.orc_pixbuf_scale(P(src), irow, sw, sh, P(want), dw * ch, dw, dh, ch, interp)
        want.setflags(write=False)
        _WANT[tag] = (src, want, rc)
    return _WANT[tag]


def row_want(orc, r, amode, k=0):
    return oracle_scale(orc, ("row", r.name, amode, k), r.sw, r.sh, r.dw, r.dh, r.ch, r.interp, pitches(r)[0], amode, 9000 + 16 * ROWS.index(r) + 4 * k + amode)


def same_bytes(got, want, what):
    bad = got != want
    assert not bad.any(), "%s: %d bytes differ from the reference, first at (row, byte) %s: got %d, want %d" % (
        what, int(bad.sum()), np.argwhere(bad)[0].tolist(), got[tuple(np.argwhere(bad)[0])], want[tuple(np.argwhere(bad)[0])])


def guarded(dh, orow):
    return dev(np.full((dh + 1, orow), FILL, np.uint8))


def frame_of(t, dw, dh, ch, what):
    """the frame bytes of a guarded destination; the guard row and the row padding must keep their fill"""
    out = host(t)
    assert (out[dh] == FILL).all(), "%s: the row past the frame was written" % what
    assert (out[:dh, dw * ch:] == FILL).all(), "%s: row padding was written" % what
    return out[:dh, :dw * ch]


def bits(ts):
    return int(np.bitwise_or.reduce([t.data_ptr() & 15 for t in ts]))


# ------------------------------------------------------------------------------------------------------------------ random geometry
Draw = namedtuple("Draw", "sw sh dw dh ch interp irow orow amode")
_DRAWS = []


def draws():
    """200 seeded scales: sw 1..300, sh 1..160, each destination side between 1/8 and 8 times its source side (log-uniform), so that the library's one-step range
    is never left; both channel counts, the three filters, pitch = row + 0 / 4 / 8 bytes rounded up to 4, the three alpha mixes"""
    if not _DRAWS:
        rng = np.random.default_rng(0x9B1A)
        while len(_DRAWS) < 200:
            sw, sh = int(rng.integers(1, 301)), int(rng.integers(1, 161))
            fx, fy = 8.0 ** rng.uniform(-1, 1), 8.0 ** rng.uniform(-1, 1)
            dw, dh = min(max(int(sw * fx), -(-sw // 8)), 8 * sw), min(max(int(sh * fy), -(-sh // 8)), 8 * sh)
            ch, interp = int(rng.choice([3, 4])), int(rng.choice([0, 2, 3, 3]))
            irow, orow = align(sw * ch + 4 * int(rng.integers(0, 3)), 4), align(dw * ch + 4 * int(rng.integers(0, 3)), 4)
            _DRAWS.append(Draw(sw, sh, dw, dh, ch, interp, irow, orow, len(_DRAWS) % 3))
    return _DRAWS


def draw_want(orc, i, dr):
    return oracle_scale(orc, ("draw", i), dr.sw, dr.sh, dr.dw, dr.dh, dr.ch, dr.interp, dr.irow, dr.amode, 12000 + i)


def test_random_draws_are_all_served(orc, ops_cpu):
    """the seed's 200 draws: the oracle refuses none, the dispatcher refuses none -- nothing is skipped -- and they spread over the families"""
    paths = {}
    assert len(draws()) == 200
    for i, dr in enumerate(draws()):
        assert dr.sw <= 8 * dr.dw and dr.dw <= 8 * dr.sw and dr.sh <= 8 * dr.dh and dr.dh <= 8 * dr.sh, dr
        assert draw_want(orc, i, dr)[2] == 0, dr
        d = ops_cpu.pixbuf_plan(dr.sw, dr.sh, dr.dw, dr.dh, dr.ch, dr.interp, irow=dr.irow, orow=dr.orow)
        assert d["path"] != "REFUSED" and d["rc"] == 0 and key(d) in REACHABLE, dr
        paths[d["path"]] = paths.get(d["path"], 0) + 1
    print("paths of the draws:", paths)
    assert {"NEAREST", "UP", "PAIRS", "WINDOW"} <= set(paths), paths


def test_the_oracle_serves_every_row(orc):
    for r in ROWS:
        assert row_want(orc, r, 0)[2] == (-2 if r.path == "REFUSED" else 0), r.name


# ------------------------------------------------------------------------------------------------------------------ GPU
def gpu_scale(gpu, src, r, flags=0, what=""):
    """lgpu_pixbuf_scale of a row's geometry into a guarded destination: (frame bytes, plan with the real pointers)"""
    irow, orow = pitches(r)
    d_src, d_dst = dev(src), guarded(r.dh, orow)
    d = plan(r, gpu, d_src.data_ptr(), d_dst.data_ptr(), mode=lib.PB_PLAN_SCALE, flags=flags)
    gpu.pixbuf_scale(d_src, d_dst, r.sw, r.sh, r.dw, r.dh, channels=r.ch, interp=r.interp | flags)
    return frame_of(d_dst, r.dw, r.dh, r.ch, what), d


SCALE_ROWS = [r for r in ROWS if r.path != "NOT_FUSED"]


@gpu_mark
@pytest.mark.parametrize("r", SCALE_ROWS, ids=lambda r: r.name)
def test_row_equals_the_oracle_on_its_kernel(gpu, orc, tune, r):
    set_tune(tune, r)
    irow, orow = pitches(r)
    if r.path == "REFUSED":
        d_src, d_dst = dev(row_want(orc, r, 0)[0]), guarded(r.dh, orow)
        assert plan(r, gpu, d_src.data_ptr(), d_dst.data_ptr())["path"] == "REFUSED"
        with pytest.raises(lib.LgpuError):
            gpu.pixbuf_scale(d_src, d_dst, r.sw, r.sh, r.dw, r.dh, channels=r.ch, interp=r.interp)
        assert (host(d_dst) == FILL).all(), "a refused scale wrote to its destination"
        return
    for amode in range(3 if r.ch == 4 else 1):
        src, want, rc = row_want(orc, r, amode)
        assert rc == 0
        got, d = gpu_scale(gpu, src, r, what=r.name)
        same_plan(d, r)
        same_bytes(got, want, "%s, alpha %s" % (describe(r, d), ALPHA_MIXES[amode]))


OPQ_ROWS = [r for r in ROWS if r.ch == 4 and r.path in ("UP", "GATHER", "PAIRS")]


@gpu_mark
@pytest.mark.parametrize("r", OPQ_ROWS, ids=lambda r: r.name)
def test_opaque_form_of_the_row(gpu, orc, tune, r):
    """LGPU_INTERP_OPAQUE on an all-255 source: the query reports the OPQ instantiation of the same plan; the bytes are the oracle's and the general form's"""
    set_tune(tune, r)
    src, want, rc = row_want(orc, r, 1)
    assert rc == 0
    got, d = gpu_scale(gpu, src, r, flags=OPAQUE, what=r.name)
    same_plan(d, r, opq=1)
    plain, d0 = gpu_scale(gpu, src, r, what=r.name)
    assert d0["opq"] == 0
    same_bytes(got, want, "opaque form, " + describe(r, d))
    same_bytes(got, plain, "opaque form against the general one, " + describe(r, d))


CHAIN_ROWS = OPQ_ROWS + [r for r in ROWS if r.path == "NOT_FUSED"]
CANVAS_ROW = "pairs4_34_pre"


def run_chain(gpu, orc, tune, r, canvas, seed, flags=0):
    """lgpu_chain_amounts on the pixbuf arithmetic: three tracks of different content, R <-> B, a blend amount per track, a LUT; fused, then staged track by track
    (PB_CHAIN_GROUP = 1).  Each track equals the oracle's stages byte for byte, both ways.  flags = OPAQUE: every source all-255, the chain carries
    LGPU_INTERP_OPAQUE and the query must name the <.., OPQ, PbEpi> form"""
    rng = np.random.default_rng(seed)
    ntr = 3
    irow = pitches(r)[0]
    cw, chh, ox, oy = canvas if canvas else (r.dw, r.dh, 0, 0)
    irow2, orow = align(cw * 4, 16) + 32, align(cw * 4, 16) + 16
    amounts = chain_ref.distinct_amounts(rng, ntr)
    lut = rng.permutation(256).astype(np.uint8)
    srcs = [make_src(rng, r.sw, r.sh, 4, irow, 1 if flags else i) for i in range(ntr)]
    l2s = [rng.integers(0, 256, (chh, irow2), dtype=np.uint8) for _ in range(ntr)]
    d_src, d_l2 = [dev(a) for a in srcs], [dev(a) for a in l2s]
    wants = [chain_ref.oracle_chain_rgba(orc, srcs[i], r.sw, r.sh, r.dw, r.dh, r.interp, 1, l2s[i], amounts[i], lut, canvas) for i in range(ntr)]
    prm = gpu.chain_params(r.sw, r.sh, irow, r.dw, r.dh, irow2, orow, swap_rb=1, interp=r.interp | PIXBUF | flags, do_blur=0, bf=99, lut=lut)
    for group in (-1, 1):
        tune("PB_CHAIN_GROUP", group)
        d_dst = [guarded(chh, orow) for _ in range(ntr)]
        doff = oy * orow + 4 * ox
        d = plan(r, gpu, bits(d_src), bits(d_dst) | (doff & 15), nframes=ntr, mode=lib.PB_PLAN_CHAIN, flags=flags)
        what = "chain%s%s, %s" % (" opaque" if flags else "", " staged" if group == 1 else "", describe(r, d))
        if group == 1:
            pass                 # the stages run apart (lgpu_pixbuf_scale_batch, then the last kernel): the chain's scale call is not made
        elif r.path == "NOT_FUSED":
            assert d["path"] == "NOT_FUSED" and d["rc"] == 0, what
        else:
            same_plan(d, r, epi=1, gz=ntr, opq=1 if flags else 0)
        gpu.chain_amounts(prm, gpu.chain_tracks(d_src, d_l2, d_dst), amounts, canvas)
        for i in range(ntr):
            same_bytes(frame_of(d_dst[i], cw, chh, 4, what), wants[i], "%s, track %d" % (what, i))


@gpu_mark
@pytest.mark.parametrize("r", CHAIN_ROWS, ids=lambda r: r.name)
def test_chain_form_of_the_row(gpu, orc, tune, r):
    set_tune(tune, r)
    run_chain(gpu, orc, tune, r, None, 10000 + ROWS.index(r))


@gpu_mark
@pytest.mark.parametrize("r", OPQ_ROWS, ids=lambda r: r.name)
def test_opaque_chain_form_of_the_row(gpu, orc, tune, r):
    """the chain with LGPU_INTERP_OPAQUE on all-255 sources: the <.., OPQ, PbEpi> instantiation of every row that has one"""
    set_tune(tune, r)
    run_chain(gpu, orc, tune, r, None, 11000 + ROWS.index(r), flags=OPAQUE)


@gpu_mark
def test_chain_row_on_a_letterbox_canvas(gpu, orc, tune):
    """the scaled frame lands at (7, 5) of a larger canvas: the fused store at an offset, the bars one more launch"""
    r = BY_NAME[CANVAS_ROW]
    set_tune(tune, r)
    run_chain(gpu, orc, tune, r, (r.dw + 19, r.dh + 8, 7, 5), 10900)


def batch_rows():
    """the first full-size row of every family"""
    seen, out = set(), []
    for r in SCALE_ROWS:
        if family(r) not in seen and r.path != "REFUSED" and not r.name.endswith(("_small", "_narrow")):
            seen.add(family(r))
            out.append(r)
    return out


def shifted(a, off):
    """a device copy of `a` whose first byte lies `off` bytes past an allocation's start"""
    flat = dev(np.concatenate([np.zeros(off, np.uint8), a.reshape(-1)]))
    return flat[off:].view(a.shape)


@gpu_mark
@pytest.mark.parametrize("r", batch_rows(), ids=lambda r: r.name)
def test_batch_of_the_row(gpu, orc, tune, r):
    """lgpu_pixbuf_scale_batch, three frames of different content, the second one the least aligned (4 bytes past a 16-byte boundary; 1 byte for 3-byte pixels):
    the exact 2:1 / 1:2 kernels, which ask for alignment, give the whole launch to another kernel -- the query with the OR of the address bits says which --
    and every frame equals its single call and the oracle"""
    set_tune(tune, r)
    irow, orow = pitches(r)
    off = 4 if r.ch == 4 else 1
    cases = [row_want(orc, r, k % 3, k) for k in range(3)]
    d_src = [shifted(c[0], off) if k == 1 else dev(c[0]) for k, c in enumerate(cases)]
    d_dst = [shifted(np.full((r.dh + 1, orow), FILL, np.uint8), off) if k == 1 else guarded(r.dh, orow) for k in range(3)]
    d = plan(r, gpu, bits(d_src), bits(d_dst), nframes=3)
    if r.path in ("DOUBLE", "HALF3", "HALF"):
        assert d["path"] in ("UP", "GATHER", "PAIRS", "WINDOW") and d["gz"] == 3, describe(r, d)
    elif r.path == "COPY":
        assert d["path"] == "COPY"
    else:
        same_plan(d, r, gz=3)
    gpu.pixbuf_scale_batch(d_src, d_dst, r.sw, r.sh, r.dw, r.dh, channels=r.ch, interp=r.interp)
    for k in range(3):
        got = frame_of(d_dst[k], r.dw, r.dh, r.ch, "%s, frame %d" % (r.name, k))
        same_bytes(got, cases[k][1], "batch, frame %d, %s" % (k, describe(r, d)))
        one = guarded(r.dh, orow)
        gpu.pixbuf_scale(d_src[k], one, r.sw, r.sh, r.dw, r.dh, channels=r.ch, interp=r.interp)
        same_bytes(got, frame_of(one, r.dw, r.dh, r.ch, r.name), "batch against the single call, frame %d, %s" % (k, describe(r, d)))


@gpu_mark
@pytest.mark.parametrize("r", [r for r in batch_rows() if r.path in ("DOUBLE", "HALF3", "HALF")], ids=lambda r: r.name)
def test_aligned_batch_of_the_exact_ratio_kernels(gpu, orc, tune, r):
    """the families a misaligned frame takes the launch away from, again with three aligned frames: k_pb_double, k_pb_half3, k_pb_half themselves on a grid of
    three frames (k_pb_half's grid is the launch's own); every frame equals the oracle"""
    set_tune(tune, r)
    irow, orow = pitches(r)
    cases = [row_want(orc, r, k % 3, k) for k in range(3)]
    d_src, d_dst = [dev(c[0]) for c in cases], [guarded(r.dh, orow) for _ in range(3)]
    d = plan(r, gpu, bits(d_src), bits(d_dst), nframes=3)
    same_plan(d, r, gz=0 if r.path == "HALF" else 3)
    gpu.pixbuf_scale_batch(d_src, d_dst, r.sw, r.sh, r.dw, r.dh, channels=r.ch, interp=r.interp)
    for k in range(3):
        same_bytes(frame_of(d_dst[k], r.dw, r.dh, r.ch, "%s, frame %d" % (r.name, k)), cases[k][1], "aligned batch, frame %d, %s" % (k, describe(r, d)))


@gpu_mark
def test_random_geometry_equals_the_oracle(gpu, orc):
    """the draws of draws(): every one served (rc 0) and byte for byte the oracle's, none skipped; prints how many draws each key received"""
    counts = {}
    for i, dr in enumerate(draws()):
        src, want, rc = draw_want(orc, i, dr)
        assert rc == 0, dr
        d_src, d_dst = dev(src), guarded(dr.dh, dr.orow)
        d = gpu.pixbuf_plan(dr.sw, dr.sh, dr.dw, dr.dh, dr.ch, dr.interp, irow=dr.irow, orow=dr.orow, src_bits=d_src.data_ptr(), dst_bits=d_dst.data_ptr())
        assert d["rc"] == 0 and d["path"] != "REFUSED", dr
        gpu.pixbuf_scale(d_src, d_dst, dr.sw, dr.sh, dr.dw, dr.dh, channels=dr.ch, interp=dr.interp)       # raises unless the call returns 0
        same_bytes(frame_of(d_dst, dr.dw, dr.dh, dr.ch, str(dr)), want, "draw %d %s, planned %s" % (i, dr, key(d)))
        counts[key(d)] = counts.get(key(d), 0) + 1
    assert sum(counts.values()) == 200
    for k in sorted(counts, key=str):
        print("%4d  %s" % (counts[k], k))
